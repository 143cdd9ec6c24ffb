"""ctypes loader of the CPU oracle (TEST INFRASTRUCTURE -- see oracle/oracle.h).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
from tracer_amd import abi  # noqa: E402  (PODs only; the oracle never calls the product path)

_LIBS = {}


def lib(libm=False):
    key = "liboracle_libm.so" if libm else "liboracle.so"
    if key not in _LIBS:
        path = os.path.join(os.environ.get("TRC_ORACLE_DIR") or _HERE, key)      # TRC_ORACLE_DIR: the sanitized build (tools/run_sanitizers.sh)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make oracle`")
        L = C.CDLL(path)
        f3 = C.POINTER(C.c_float)
        L.orc_uses_libm.restype = C.c_int
        L.orc_pcg32_srandom.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64, C.c_uint64]
        L.orc_pcg32_srandom.restype = None
        L.orc_pcg32_random.argtypes = [C.POINTER(C.c_uint64), C.c_uint64]
        L.orc_pcg32_random.restype = C.c_uint32
        L.orc_randomF.argtypes = [C.POINTER(C.c_uint64), C.c_uint64]
        L.orc_randomF.restype = C.c_float
        L.orc_trace_rays.argtypes = [C.POINTER(abi.Scene), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
        L.orc_trace_rays.restype = None
        L.orc_trace_rays_brute.argtypes = [C.POINTER(abi.Scene), C.c_void_p, C.c_size_t, C.c_void_p]
        L.orc_trace_rays_brute.restype = None
        L.orc_render.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Camera), f3, C.c_uint32, C.c_uint32,
                                 C.c_void_p, C.c_void_p, C.POINTER(abi.Params), C.POINTER(abi.Stats), C.c_int]
        L.orc_render.restype = None
        L.orc_material_S_F.argtypes = [C.POINTER(abi.Material), f3, f3, f3, f3, f3, f3]
        L.orc_material_S_F.restype = None
        L.orc_material_F.argtypes = [C.POINTER(abi.Material), f3, f3, f3, f3, f3, f3]
        L.orc_material_F.restype = None
        L.orc_material_PDF.argtypes = [C.POINTER(abi.Material), f3, f3, f3]
        L.orc_material_PDF.restype = C.c_float
        L.orc_offset_ray.argtypes = [f3, f3, f3]
        L.orc_offset_ray.restype = None
        L.orc_fr_dielectric.argtypes = [C.c_float, C.c_float]
        L.orc_fr_dielectric.restype = C.c_float
        L.orc_fr_conductor.argtypes = [C.c_float, f3, f3, f3]
        L.orc_fr_conductor.restype = None
        L.orc_power_heuristic.argtypes = [C.c_int, C.c_float, C.c_int, C.c_float]
        L.orc_power_heuristic.restype = C.c_float
        L.orc_sobol_interval_to_index.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
        L.orc_sobol_interval_to_index.restype = C.c_uint64
        L.orc_sobol_sample_float.argtypes = [C.c_uint64, C.c_uint32]
        L.orc_sobol_sample_float.restype = C.c_float
        L.orc_sobol_sample_dimension.argtypes = [C.c_uint32] * 6
        L.orc_sobol_sample_dimension.restype = C.c_float
        L.orc_cosine_sample_hemisphere.argtypes = [f3, f3]
        L.orc_cosine_sample_hemisphere.restype = None
        L.orc_erf.argtypes = [C.c_float]
        L.orc_erf.restype = C.c_float
        L.orc_erfinv.argtypes = [C.c_float]
        L.orc_erfinv.restype = C.c_float
        L.orc_aabb_hit_t.argtypes = [C.POINTER(abi.AABB), C.POINTER(abi.Ray), C.c_float, C.c_float,
                                     C.POINTER(C.c_float)]
        L.orc_aabb_hit_t.restype = C.c_int
        L.orc_cast_ray.argtypes = [C.POINTER(abi.Camera), C.c_float, C.c_float, C.POINTER(C.c_uint64), C.c_uint64,
                                   f3, f3]
        L.orc_cast_ray.restype = None
        L.orc_sppm_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
        L.orc_sppm_create.restype = C.c_void_p
        L.orc_sppm_destroy.argtypes = [C.c_void_p]
        L.orc_sppm_destroy.restype = None
        L.orc_sppm_frames.argtypes = [C.c_void_p, C.POINTER(abi.Scene), C.POINTER(abi.Camera), f3, C.c_void_p,
                                      C.c_void_p, C.c_uint32]
        L.orc_sppm_frames.restype = None
        L.orc_sppm_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(abi.Complex)]
        L.orc_sppm_download.restype = None
        L.orc_photon_hash.argtypes = [f3, C.c_float]
        L.orc_photon_hash.restype = C.c_float
        L.orc_hg_sample.argtypes = [C.c_float, f3, f3, f3]
        L.orc_hg_sample.restype = C.c_float
        L.orc_phase_hg.argtypes = [C.c_float, C.c_float]
        L.orc_phase_hg.restype = C.c_float
        L.orc_grid_density.argtypes = [C.POINTER(abi.GridDensityInfo), C.c_void_p, f3]
        L.orc_grid_density.restype = C.c_float
        L.orc_tonemap.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_float)]
        L.orc_tonemap.restype = None
        L.orc_set_environment_map.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        L.orc_set_environment_map.restype = None
        L.orc_set_density.argtypes = [C.POINTER(abi.GridDensityInfo), C.c_void_p]
        L.orc_set_density.restype = None
        L.orc_set_triangle_materials.argtypes = [C.c_void_p, C.c_uint32]
        L.orc_set_triangle_materials.restype = None
        L.orc_set_textures.argtypes = [C.c_void_p, C.c_uint32]
        L.orc_set_textures.restype = None
        L.orc_set_mesh_light_pick.argtypes = [C.c_int]
        L.orc_set_mesh_light_pick.restype = None
        L.orc_debug_branch_counts.argtypes = [C.c_void_p, C.c_int]
        L.orc_debug_branch_counts.restype = None
        L.orc_debug_branch_name.argtypes = [C.c_uint32]
        L.orc_debug_branch_name.restype = C.c_char_p
        L.orc_lbvh_build.argtypes = [C.POINTER(abi.BVH), C.c_uint32, C.POINTER(abi.BVH), C.POINTER(C.c_uint32)]
        L.orc_lbvh_build.restype = None
        L.orc_sah_build.argtypes = [C.POINTER(abi.BVH), C.c_uint32, C.POINTER(abi.BVH)]
        L.orc_sah_build.restype = None
        L.orc_sah_leaf.argtypes = [C.POINTER(abi.AABB), C.POINTER(abi.float4x4), C.c_int32, C.c_uint32, C.POINTER(abi.BVH)]
        L.orc_sah_leaf.restype = None
        L.orc_math.argtypes = [C.c_int, C.c_float, C.c_float]
        L.orc_math.restype = C.c_float
        _LIBS[key] = L
    return _LIBS[key]


RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("tmax", np.float32), ("direction", np.float32, 3),
                      ("_pad", np.uint32)])
HIT_DTYPE = np.dtype([("hit", np.int32), ("pType", np.int32), ("pIndex", np.uint32), ("t", np.float32),
                      ("p", np.float32, 3), ("gn", np.float32, 3), ("sn", np.float32, 3), ("uv", np.float32, 2),
                      ("material", np.uint32), ("PDF", np.float32),
                      ("n_descend", np.uint32), ("n_return", np.uint32), ("n_leaf", np.uint32)])
assert RAY_DTYPE.itemsize == C.sizeof(abi.Ray) and HIT_DTYPE.itemsize == C.sizeof(abi.Hit)


def make_rays(origins, directions, tmax=None):
    n = len(origins)
    rays = np.zeros(n, dtype=RAY_DTYPE)
    rays["origin"] = origins
    rays["direction"] = directions
    rays["tmax"] = np.float32(np.finfo(np.float32).max) if tmax is None else tmax
    return rays


def trace_rays(scene_view, rays, any_hit=False, brute=False, libm=False, triangle_materials=None):
    hits = np.zeros(len(rays), dtype=HIT_DTYPE)
    L = lib(libm)
    with _features(L, triangle_materials):
        if brute:
            L.orc_trace_rays_brute(C.byref(scene_view), rays.ctypes.data, len(rays), hits.ctypes.data)
        else:
            L.orc_trace_rays(C.byref(scene_view), rays.ctypes.data, len(rays), hits.ctypes.data, 1 if any_hit else 0)
    return hits


def render(scene_view, camera, width, height, rng, accum=None, spp=1, max_depth=8, integrator=0, frame0=0,
           env=(0.0, 0.0, 0.0), tile_rank=0, tile_nranks=1, n_threads=0, libm=False, view_height=0, sobol=False,
           env_light=False, mesh_lights=False, mesh_light_pick=1, triangle_materials=None, textures=None):
    """kernelPathTracing on the CPU.  rng: (H,W,4) uint32, updated in place.  Returns (accum, stats).
    The project's own features (include/tracer_abi.h; not the reference's), for this call only: env_light = TRC_FLAG_ENV_LIGHT over
    the map of set_environment_map, mesh_lights = TRC_FLAG_MESH_LIGHTS (mesh_light_pick: the knob of that name), both traceMIS
    without Sobol'; triangle_materials = the array of trc_upload_triangle_materials; textures = the images of trc_upload_textures,
    (h, w, 3) float32 each, rows bottom-up."""
    assert rng.dtype == np.uint32 and rng.shape == (height, width, 4) and rng.flags.c_contiguous
    if accum is None:
        accum = np.zeros((height, width, 4), dtype=np.float32)
    assert accum.dtype == np.float32 and accum.shape == (height, width, 4) and accum.flags.c_contiguous
    assert not (env_light and mesh_lights), "one light besides the squares, never two"
    if env_light or mesh_lights:
        assert integrator == abi.INTEGRATOR_MIS and not sobol, "the light flags are traceMIS's, without Sobol'"
    assert not env_light or _ENVMAP_KEEPALIVE, "TRC_FLAG_ENV_LIGHT needs a map (set_environment_map)"
    flags = abi.FLAG_COLLECT_STATS | (abi.FLAG_SOBOL if sobol else 0)
    flags |= (abi.FLAG_ENV_LIGHT if env_light else 0) | (abi.FLAG_MESH_LIGHTS if mesh_lights else 0)
    prm = abi.Params(spp=spp, max_depth=max_depth, integrator=integrator, frame0=frame0,
                     tile_rank=tile_rank, tile_nranks=tile_nranks, flags=flags, view_height=view_height)
    stats = abi.Stats()
    env_c = (C.c_float * 3)(*env)
    L = lib(libm)
    with _features(L, triangle_materials, textures, mesh_light_pick):
        L.orc_render(C.byref(scene_view), C.byref(camera), env_c, width, height, rng.ctypes.data,
                     accum.ctypes.data, C.byref(prm), C.byref(stats), n_threads)
    return accum, stats


class _features:
    """per-triangle materials, image textures and the mesh_light_pick knob set in the oracle for the calls inside the block"""

    def __init__(self, L, triangle_materials=None, textures=None, mesh_light_pick=1):
        self.L, self.pick = L, mesh_light_pick
        self.tm = None if triangle_materials is None else np.ascontiguousarray(triangle_materials, dtype=np.uint32)
        self.imgs = None
        if textures:
            self.texels = [np.ascontiguousarray(t, dtype=np.float32) for t in textures]
            assert all(t.ndim == 3 and t.shape[2] == 3 and t.size for t in self.texels)
            self.imgs = (abi.Image * len(self.texels))()
            for d, t in zip(self.imgs, self.texels):
                d.width, d.height, d.rgb = t.shape[1], t.shape[0], t.ctypes.data_as(C.POINTER(C.c_float))

    def __enter__(self):
        if self.tm is not None:
            self.L.orc_set_triangle_materials(self.tm.ctypes.data, len(self.tm))
        if self.imgs is not None:
            self.L.orc_set_textures(C.cast(self.imgs, C.c_void_p), len(self.imgs))
        self.L.orc_set_mesh_light_pick(int(self.pick))

    def __exit__(self, *exc):
        self.L.orc_set_triangle_materials(None, 0)
        self.L.orc_set_textures(None, 0)
        self.L.orc_set_mesh_light_pick(1)


BRANCHES = None


def branch_counts(reset=False, libm=False):
    """visits of traceMISLight's branches (oracle.h: orc_branch) since the last reset -> {name: count}"""
    global BRANCHES
    L = lib(libm)
    if BRANCHES is None:
        BRANCHES = []
        while L.orc_debug_branch_name(len(BRANCHES)):
            BRANCHES.append(L.orc_debug_branch_name(len(BRANCHES)).decode())
    out = np.zeros(len(BRANCHES), dtype=np.uint64)
    L.orc_debug_branch_counts(out.ctypes.data, 1 if reset else 0)
    return dict(zip(BRANCHES, (int(c) for c in out)))


def shard_seed(seed, sample_group):
    """Seed of sample group g of a sample-sharded frame (include/tracer_abi.h, "sample sharding"): the golden-ratio
    stride 0x9E3779B97F4A7C15 times g is added modulo 2^64, so group 0 renders the unsharded frame's first samples."""
    return (seed + sample_group * 0x9E3779B97F4A7C15) % (1 << 64)


def render_sample_sharded(scene_view, camera, width, height, rngs, spp, **kw):
    """The sample-sharded frame as include/tracer_abi.h defines it, on the CPU: group g renders the whole frame with
    spp / S samples (frame0 = 0) from ITS RNG texture rngs[g] (= fillRNG of shard_seed(seed, g), S = len(rngs)); the
    composed texel is (((A_0 + A_1) + A_2) + ...) / float32(S) in binary32, channel by channel.  kw: render()'s
    (integrator, max_depth, env, tile_rank / tile_nranks to restrict the pixels, n_threads ...).
    Returns (composed, [stats per group])."""
    S = len(rngs)
    assert S >= 1 and spp % S == 0, "every group renders the same number of samples"
    total, stats = None, []
    for g in range(S):
        a, st = render(scene_view, camera, width, height, rngs[g], spp=spp // S, frame0=0, **kw)
        stats.append(st)
        total = a if total is None else np.add(total, a, dtype=np.float32)
    return np.divide(total, np.float32(S), dtype=np.float32), stats


def tonemap(accum):
    """fragmentShader's exposure + ACES on an (H, W, 4) float32 accumulator -> ((H, W, 4) uint8 top-down, exposure)."""
    assert accum.dtype == np.float32 and accum.ndim == 3 and accum.shape[2] == 4 and accum.flags.c_contiguous
    H, W = accum.shape[:2]
    out = np.empty((H, W, 4), dtype=np.uint8)
    e = C.c_float(0)
    lib().orc_tonemap(accum.ctypes.data, W, H, out.ctypes.data, C.byref(e))
    return out, e.value


_ENVMAP_KEEPALIVE = []


def set_environment_map(rgb):
    """(h, w, 3) float32 equirectangular environment, or None for the constant one."""
    _ENVMAP_KEEPALIVE.clear()
    for libm in (False, True):
        if rgb is None:
            lib(libm).orc_set_environment_map(0, 0, None)
        else:
            assert rgb.dtype == np.float32 and rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.flags.c_contiguous
            lib(libm).orc_set_environment_map(rgb.shape[1], rgb.shape[0], rgb.ctypes.data)
    if rgb is not None:
        _ENVMAP_KEEPALIVE.append(rgb)


_DENSITY_KEEPALIVE = []


def set_density(info, density):
    """Density grid for integrator 2 (traceVolume); `density`: float32 array (nz, ny, nx) or None to clear."""
    _DENSITY_KEEPALIVE.clear()
    for libm in (False, True):
        if density is None:
            lib(libm).orc_set_density(None, None)
        else:
            assert density.dtype == np.float32 and density.flags.c_contiguous
            lib(libm).orc_set_density(C.byref(info), density.ctypes.data)
    if density is not None:
        _DENSITY_KEEPALIVE.append(density)


def lbvh_build(leaves, n):
    """LBVH over `n` leaf records (ctypes array / pointer of abi.BVH) -> (abi.BVH * (2n-1), height)."""
    out = (abi.BVH * (2 * n - 1))()
    h = C.c_uint32(0)
    lib().orc_lbvh_build(leaves, n, out, C.byref(h))
    return out, h.value


def sah_build(leaves, n):
    """The reference's SAH build (BVH.hh:35-269) over `n` leaf records -> abi.BVH * (2n-1), root first."""
    out = (abi.BVH * (2 * n - 1))()
    lib().orc_sah_build(leaves, n, out)
    return out


def sah_leaf(box, model_matrix, ptype, pindex):
    """BVH::buildNode (BVH.hh:273-314) -> abi.BVH leaf record."""
    out = abi.BVH()
    lib().orc_sah_leaf(C.byref(box), C.byref(model_matrix), ptype, pindex, C.byref(out))
    return out


CAMREC_DTYPE = np.dtype([("ratio", np.float32, 4), ("position", np.float32, 4), ("direction", np.float32, 4),
                         ("valid", np.uint8), ("_pad0", np.uint8, 15), ("alternative", np.float32, 4),
                         ("flux", np.float32, 4), ("radius", np.float32), ("photonCount", np.uint32),
                         ("_pad1", np.uint32, 2)])
PHOTON_DTYPE = np.dtype([("flux", np.float32, 4), ("normal", np.float32, 4), ("position", np.float32, 4),
                         ("direction", np.float32, 4), ("step", np.uint8), ("active", np.uint8), ("_pad", np.uint8, 14)])
assert CAMREC_DTYPE.itemsize == 112 and PHOTON_DTYPE.itemsize == 80


class Sppm:
    """SPPM pass on the CPU oracle (Photon.metal); canvas rng / accum are updated in place."""

    def __init__(self, width, height, photon_seed):
        self.W, self.H = width, height
        self._h = lib().orc_sppm_create(width, height, photon_seed)

    def frames(self, scene_view, camera, rng, accum, n_frames=1, env=(0.0, 0.0, 0.0), triangle_materials=None, textures=None):
        assert rng.dtype == np.uint32 and rng.shape == (self.H, self.W, 4) and rng.flags.c_contiguous
        assert accum.dtype == np.float32 and accum.shape == (self.H, self.W, 4) and accum.flags.c_contiguous
        with _features(lib(), triangle_materials, textures):
            lib().orc_sppm_frames(self._h, C.byref(scene_view), C.byref(camera), (C.c_float * 3)(*env), rng.ctypes.data,
                                  accum.ctypes.data, n_frames)

    def download(self):
        n = abi.PHOTON_HASHN
        cam = np.zeros(self.W * self.H, dtype=CAMREC_DTYPE)
        pho = np.zeros(n * n, dtype=PHOTON_DTYPE)
        mark = np.zeros((n, n, 4), dtype=np.float32)
        count = np.zeros((n, n), dtype=np.float32)
        cx = abi.Complex()
        lib().orc_sppm_download(self._h, cam.ctypes.data, pho.ctypes.data, mark.ctypes.data, count.ctypes.data, C.byref(cx))
        return cam, pho, mark, count, cx

    def __del__(self):
        if getattr(self, "_h", None):
            lib().orc_sppm_destroy(self._h)
            self._h = None


# ---------------------------------------------------------------------------------------------------------------------
# pin_api.h: the unit entry points that exist twice, orc_* here and ref_* in _ref/libmetal_ref.so (the reference's own
# shader headers compiled on the host).  Pin binds one family; tests/reference_pin_cases.py drives both the same way.
PIN_RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("direction", np.float32, 3), ("range", np.float32, 2)])
PIN_REC_DTYPE = np.dtype([("accepted", np.int32), ("range_y", np.float32), ("t", np.float32), ("p", np.float32, 3),
                          ("gn", np.float32, 3), ("sn", np.float32, 3), ("uv", np.float32, 2), ("material", np.uint32),
                          ("PDF", np.float32), ("f", np.int32)])
assert PIN_RAY_DTYPE.itemsize == 32 and PIN_REC_DTYPE.itemsize == 68
METAL_REF = os.path.join(_HERE, "_ref", "libmetal_ref.so")


def pin_rays(origin, direction, lo, hi):
    r = np.zeros(len(origin), dtype=PIN_RAY_DTYPE)
    r["origin"], r["direction"] = origin, direction
    r["range"][:, 0], r["range"][:, 1] = lo, hi
    return r


class Pin:
    """One family of pin_api.h: Pin() is orc_* of liboracle.so, Pin(ref=True) is ref_* of _ref/libmetal_ref.so."""

    def __init__(self, ref=False):
        self.prefix = "ref" if ref else "orc"
        if ref:
            if not os.path.exists(METAL_REF):
                raise RuntimeError(f"{METAL_REF} is missing: `make -C oracle` builds it where the reference is present")
            self.L = C.CDLL(METAL_REF)
        else:
            self.L = lib()
        v, z, i, f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
        sig = {"literal_probe": ([f, f], f), "gamma": ([i], f),
               "sphere_hit": [v, z, v, z, v], "square_hit": [v, z, v, z, v], "cube_hit": [v, z, v, z, v], "triangle_hit": [v, z, v, z, v],
               "aabb_hit": [v, z, v, z, v], "aabb_hit_t_n": [v, z, v, z, v, v], "aabb_hit_record": [v, z, v, z, v],
               "scene_hit": [C.POINTER(abi.Scene), v, z, i, v],
               "square_sample": [v, z, v, v, z, v], "triangle_sample": [v, z, v, z, v], "triangle_area": [v, z, v],
               "offset_ray_n": [v, v, z, v], "next_float_up": [v, z, v], "next_float_down": [v, z, v], "erf_n": [v, z, v], "erfinv_n": [v, z, v],
               "cosine_sample_hemisphere_n": [v, z, v], "concentric_sample_disk": [v, z, v], "uniform_sample_triangle": [v, z, v],
               "power_heuristic_n": [i, v, i, v, z, v], "coordinate_system": [v, z, v], "spherical_direction": [v, v, z, v],
               "phase_hg_n": [v, v, z, v], "hg_sample_n": [v, v, v, z, v],
               "fr_dielectric_n": [v, v, z, v], "fr_conductor_n": [v, v, v, z, v], "reflect": [v, v, z, v], "refract": [v, v, v, z, v],
               "material_f_n": [C.POINTER(abi.Material), v, v, v, v, z, v], "material_pdf_n": [C.POINTER(abi.Material), v, v, v, z, v],
               "material_s_f_n": [C.POINTER(abi.Material), v, v, v, z, v], "microfacet": [i, f, f, v, v, v, z, v]}
        self._fn = {}
        for name, s in sig.items():
            fn = getattr(self.L, f"{self.prefix}_{name}")
            fn.argtypes, fn.restype = (s[0], s[1]) if isinstance(s, tuple) else (s, None)
            self._fn[name] = fn

    @staticmethod
    def _f(a, width=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert width is None or (a.ndim == 2 and a.shape[1] == width) or (width == 1 and a.ndim == 1), (a.shape, width)
        return a

    def literal_probe(self, u, v):
        return np.float32(self._fn["literal_probe"](float(u), float(v)))

    def gamma(self, n):
        return np.float32(self._fn["gamma"](int(n)))

    def _prims(self, prims, T):
        """prims: a ctypes array of T (or of TriangleVertex, 3 per triangle)"""
        assert isinstance(prims, C.Array) and prims._type_ is T
        return C.addressof(prims), len(prims)

    def hit(self, kind, prims, rays):
        """kind: sphere / square / cube / triangle / aabb_record -> PIN_REC_DTYPE array"""
        T = {"sphere": abi.Sphere, "square": abi.Square, "cube": abi.Cube, "triangle": abi.TriangleVertex, "aabb_record": abi.AABB}[kind]
        addr, n_prim = self._prims(prims, T)
        n_prim = n_prim // 3 if kind == "triangle" else n_prim
        assert rays.dtype == PIN_RAY_DTYPE and rays.flags.c_contiguous and n_prim > 0
        out = np.zeros(len(rays), dtype=PIN_REC_DTYPE)
        self._fn["aabb_hit_record" if kind == "aabb_record" else kind + "_hit"](addr, n_prim, rays.ctypes.data, len(rays), out.ctypes.data)
        return out

    def aabb_hit(self, boxes, rays):
        addr, n_prim = self._prims(boxes, abi.AABB)
        out = np.zeros(len(rays), dtype=np.int32)
        self._fn["aabb_hit"](addr, n_prim, rays.ctypes.data, len(rays), out.ctypes.data)
        return out

    def aabb_hit_t(self, boxes, rays):
        addr, n_prim = self._prims(boxes, abi.AABB)
        out, t = np.zeros(len(rays), dtype=np.int32), np.zeros(len(rays), dtype=np.float32)
        self._fn["aabb_hit_t_n"](addr, n_prim, rays.ctypes.data, len(rays), out.ctypes.data, t.ctypes.data)
        return out, t

    def scene_hit(self, scene_view, rays, any_hit=False):
        assert rays.dtype == RAY_DTYPE and rays.flags.c_contiguous
        out = np.zeros(len(rays), dtype=PIN_REC_DTYPE)
        self._fn["scene_hit"](C.byref(scene_view), rays.ctypes.data, len(rays), 1 if any_hit else 0, out.ctypes.data)
        return out

    def square_sample(self, squares, u, pos):
        addr, n_prim = self._prims(squares, abi.Square)
        u, pos = self._f(u, 2), self._f(pos, 3)
        out = np.zeros((len(u), 8), dtype=np.float32)
        self._fn["square_sample"](addr, n_prim, u.ctypes.data, pos.ctypes.data, len(u), out.ctypes.data)
        return out

    def triangle_sample(self, verts, u):
        addr, nv = self._prims(verts, abi.TriangleVertex)
        u = self._f(u, 2)
        out = np.zeros((len(u), 7), dtype=np.float32)
        self._fn["triangle_sample"](addr, nv // 3, u.ctypes.data, len(u), out.ctypes.data)
        return out

    def triangle_area(self, verts):
        addr, nv = self._prims(verts, abi.TriangleVertex)
        out = np.zeros(nv // 3, dtype=np.float32)
        self._fn["triangle_area"](addr, nv // 3, out.ctypes.data)
        return out

    def map(self, name, out_width, *inputs):
        """the plain array functions: inputs are (n,) or (n, w) float32 arrays in the order of the C signature -> (n, out_width)"""
        arrs = [self._f(a) for a in inputs]
        n = len(arrs[0])
        assert all(len(a) == n for a in arrs)
        out = np.zeros((n, out_width), dtype=np.float32)
        self._fn[name](*[a.ctypes.data for a in arrs], n, out.ctypes.data)
        return out

    def power_heuristic(self, nf, f_pdf, ng, g_pdf):
        f_pdf, g_pdf = self._f(f_pdf), self._f(g_pdf)
        out = np.zeros((len(f_pdf), 1), dtype=np.float32)
        self._fn["power_heuristic_n"](nf, f_pdf.ctypes.data, ng, g_pdf.ctypes.data, len(f_pdf), out.ctypes.data)
        return out

    def material(self, which, m, *inputs):
        """which: f (wo wi uv uu -> f[3] pdf), pdf (wo wi uu -> pdf), s_f (wo uv uu -> wi[3] f[3] pdf)"""
        arrs = [self._f(a) for a in inputs]
        n = len(arrs[0])
        out = np.zeros((n, {"f": 4, "pdf": 1, "s_f": 7}[which]), dtype=np.float32)
        self._fn[f"material_{which}_n"](C.byref(m), *[a.ctypes.data for a in arrs], n, out.ctypes.data)
        return out

    def microfacet(self, dist, ax, ay, wo, wh, uu):
        wo, wh, uu = self._f(wo, 3), self._f(wh, 3), self._f(uu, 2)
        out = np.zeros((len(wo), 8), dtype=np.float32)
        self._fn["microfacet"](dist, ax, ay, wo.ctypes.data, wh.ctypes.data, uu.ctypes.data, len(wo), out.ctypes.data)
        return out
