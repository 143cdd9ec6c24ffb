"""Wraps tests/meshlight_ref/meshlight_ref.cpp (the CPU restatement of TRC_FLAG_MESH_LIGHTS' light set, tables and sampler), which the
oracle library links in (oracle/Makefile)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Ref:
    def __init__(self, L):
        self.L = L

    def tables(self, tri_v, tri_mat, mat_type, mat_albedo):
        """tri_v (n, 3, 3) float32 vertices per triangle as uploaded, tri_mat (n,) material per triangle, mat_type (m,) and mat_albedo
        (m, 3): the material table -> dict(alias (n_lights, 2), tri (n_lights,), pdfA (n,), total, n_lights, tri_v)"""
        tri_v = np.ascontiguousarray(tri_v, dtype=np.float32).reshape(-1, 3, 3)
        tri_mat = np.ascontiguousarray(tri_mat, dtype=np.uint32)
        mat_type = np.ascontiguousarray(mat_type, dtype=np.int32)
        mat_albedo = np.ascontiguousarray(mat_albedo, dtype=np.float32).reshape(-1, 3)
        n = tri_v.shape[0]
        assert tri_mat.shape == (n,) and mat_albedo.shape[0] == mat_type.shape[0]
        alias = np.zeros((max(n, 1), 2), np.uint32)
        tri = np.zeros(max(n, 1), np.uint32)
        pdfA = np.zeros(n, np.float32)
        total, nl = C.c_double(), C.c_uint32()
        self.L.meshlight_ref_tables(tri_v.ctypes.data, n, tri_mat.ctypes.data, mat_type.ctypes.data, mat_albedo.ctypes.data, mat_type.shape[0],
                                    alias.ctypes.data, tri.ctypes.data, pdfA.ctypes.data, C.byref(total), C.byref(nl))
        return dict(alias=np.ascontiguousarray(alias[:nl.value]), tri=np.ascontiguousarray(tri[:nl.value]), pdfA=pdfA, total=total.value,
                    n_lights=nl.value, tri_v=tri_v)

    def sample(self, t, draws, pos):
        draws = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1, 4)
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        assert t["n_lights"] > 0 and draws.shape[0] == pos.shape[0]
        tri = np.empty(draws.shape[0], np.uint32)
        out = np.empty((draws.shape[0], 7), np.float32)
        self.L.meshlight_ref_sample(t["tri_v"].ctypes.data, t["alias"].ctypes.data, t["tri"].ctypes.data, t["pdfA"].ctypes.data, t["n_lights"],
                                    draws.ctypes.data, pos.ctypes.data, draws.shape[0], tri.ctypes.data, out.ctypes.data)
        return tri, out


def build():
    """the restatement as the oracle library holds it (oracle/Makefile links tests/meshlight_ref/meshlight_ref.cpp into liboracle.so: one CPU
    statement, one build of it).  make runs every time -- it does nothing when the library is newer than its sources -- so an edit of the
    restatement is never answered from a stale library; TRC_ORACLE_DIR names a build of somebody else's making (the sanitized one)."""
    if os.environ.get("TRC_ORACLE_DIR"):
        so = os.path.join(os.environ["TRC_ORACLE_DIR"], "liboracle.so")
    else:
        so = os.path.join(ROOT, "oracle", "liboracle.so")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle.so"], stdout=subprocess.DEVNULL)
    L = C.CDLL(so)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    L.meshlight_ref_tables.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(u32)]
    L.meshlight_ref_tables.restype = None
    L.meshlight_ref_sample.argtypes = [vp, vp, vp, vp, u32, vp, vp, sz, vp, vp]
    L.meshlight_ref_sample.restype = None
    return Ref(L)


def tri_areas(tri_v):
    """float64 areas of (n, 3, 3) triangles (for the tests' own arithmetic, not the restatement's)"""
    v = np.asarray(tri_v, dtype=np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def edge_draws(rng, n):
    """(n, 4) uint32 draws: the edge values r in {0, 1, 2^31, 2^32 - 1} and f in {0, 2^-32, 1 - 2^-24, 1} in every combination, then random ones"""
    rs = np.array([0, 1, 1 << 31, (1 << 32) - 1], np.uint32)
    fs = np.array([0.0, 2.0 ** -32, 1.0 - 2.0 ** -24, 1.0], np.float32).view(np.uint32)
    grid = np.array([[a, b, c, d] for a in rs for b in rs for c in fs for d in fs], np.uint32)
    m = max(0, n - grid.shape[0])
    r = rng.integers(0, 1 << 32, size=(m, 2), dtype=np.uint64).astype(np.uint32)
    f = np.ldexp(rng.integers(0, 1 << 32, size=(m, 2), dtype=np.uint64).astype(np.float32), -32).astype(np.float32).view(np.uint32)
    return np.ascontiguousarray(np.concatenate([grid, np.concatenate([r, f], axis=1)], axis=0))


def view_triangles(view):
    """(n, 3, 3) float32: the vertices of every triangle of a scene view, as uploaded (triList gathered through idxList)"""
    n_v, n_i = view.n_vertex, view.n_index
    if n_i == 0:
        return np.zeros((0, 3, 3), np.float32)
    v = np.ctypeslib.as_array(C.cast(view.triList, C.POINTER(C.c_float)), shape=(n_v, 8))
    i = np.ctypeslib.as_array(view.idxList, shape=(n_i,))
    return np.ascontiguousarray(v[i.astype(np.int64), :3].reshape(-1, 3, 3), dtype=np.float32)


def view_materials(view):
    """(type (m,) int32, albedo (m, 3) float32) of a scene view's material table"""
    m = view.n_material
    ty = np.array([view.materials[k].type for k in range(m)], np.int32)
    al = np.array([[view.materials[k].textureInfo.albedo.x, view.materials[k].textureInfo.albedo.y, view.materials[k].textureInfo.albedo.z]
                   for k in range(m)], np.float32).reshape(m, 3)
    return ty, al


def alias_probabilities(tab):
    """probability of every entry of an alias table ({threshold, alias} pairs), exactly as the sampler's integer draws give it"""
    n = tab.shape[0]
    keep = tab[:, 0].astype(np.float64) / 2.0 ** 32
    p = keep / n
    np.add.at(p, tab[:, 1].astype(np.int64), (1.0 - keep) / n)
    return p
