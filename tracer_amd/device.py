"""Device side: the HIP path tracer behind the C ABI (libtracer_amd.so, gfx950).

`Tracer` plays the role of the reference's AAPLRenderer for the path-tracing path
(RT_Metal/Tracer/AAPLRenderer.hh:7-14: init / render); every method is one trc_* call of
include/tracer_abi.h.  There is NO CPU fallback: a missing library or a missing GPU raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_LIB = None
_LIB_FAST = None
_LIB_HOOKS = None


class TracerError(RuntimeError):
    def __init__(self, what, status, detail=""):
        super().__init__(f"{what}: trc_status {status}" + (f" ({detail})" if detail else ""))
        self.status = status


def lib_path():
    """The in-tree build; TRC_AMD_LIB points the A/B tools (tools/ab_bench.py) at another build of the same library."""
    return os.environ.get("TRC_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libtracer_amd.so")


def fast_lib_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libtracer_amd_fast.so")


def hooks_lib_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libtracer_amd_hooks.so")


def lib(fast_math=False, hooks=False):
    """Load libtracer_amd.so (fails loudly when the HIP extension has not been built); fast_math=True loads the
    fast-math build of the same sources (libtracer_amd_fast.so) instead; hooks=True the build that also exports the test
    hooks of include/tracer_test_hooks.h (libtracer_amd_hooks.so: tests and tools only)."""
    global _LIB, _LIB_FAST, _LIB_HOOKS
    if hooks:
        if _LIB_HOOKS is None:
            _LIB_HOOKS = _load(hooks_lib_path(), hooks=True)
            assert _LIB_HOOKS.trc_has_test_hooks() == 1
        return _LIB_HOOKS
    if fast_math:
        if _LIB_FAST is None:
            _LIB_FAST = _load(fast_lib_path())
            assert _LIB_FAST.trc_build_flavor() == b"fast-math"
        return _LIB_FAST
    if _LIB is None:
        _LIB = _load(lib_path())
    return _LIB


def _load(path, hooks=False):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: the HIP extension is not built "
                           f"(run `make hip` or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(path)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    L.trc_abi_version.restype = u32
    L.trc_build_flavor.restype = C.c_char_p
    L.trc_status_string.argtypes = [i32]
    L.trc_status_string.restype = C.c_char_p
    L.trc_last_error.argtypes = [vp]
    L.trc_last_error.restype = C.c_char_p
    L.trc_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.trc_destroy.argtypes = [vp]
    L.trc_destroy.restype = None
    L.trc_upload_scene.argtypes = [vp, C.POINTER(abi.Scene)]
    L.trc_set_environment_map.argtypes = [vp, u32, u32, vp]
    L.trc_tonemap.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.trc_upload_density.argtypes = [vp, C.POINTER(abi.GridDensityInfo), vp]
    L.trc_upload_scene_lbvh.argtypes = [vp, C.POINTER(abi.Scene)]
    L.trc_upload_scene_sah.argtypes = [vp, C.POINTER(abi.Scene)]
    L.trc_upload_scene_device.argtypes = [vp, C.POINTER(abi.Scene), u32]
    L.trc_download_bvh.argtypes = [vp, C.POINTER(abi.BVH), u32, C.POINTER(u32)]
    L.trc_lbvh_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_float)]
    L.trc_set_camera.argtypes = [vp, C.POINTER(abi.Camera)]
    L.trc_set_environment.argtypes = [vp, C.POINTER(C.c_float)]
    L.trc_resize.argtypes = [vp, u32, u32]
    L.trc_seed.argtypes = [vp, u64]
    for name in ("trc_upload_rng", "trc_download_rng", "trc_upload_accum", "trc_download_accum"):
        getattr(L, name).argtypes = [vp, vp]
    L.trc_clear_accum.argtypes = [vp]
    L.trc_render.argtypes = [vp, C.POINTER(abi.Params)]
    L.trc_synchronize.argtypes = [vp]
    L.trc_trace_rays.argtypes = [vp, vp, C.c_size_t, vp, C.c_int]
    L.trc_get_stats.argtypes = [vp, C.POINTER(abi.Stats)]
    L.trc_reset_stats.argtypes = [vp]
    L.trc_sppm_init.argtypes = [vp, u64]
    L.trc_sppm_frames.argtypes = [vp, u32]
    L.trc_sppm_download.argtypes = [vp, vp, vp, vp, vp, C.POINTER(abi.Complex)]
    L.trc_device_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.trc_group_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    L.trc_group_init.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int, C.c_int]
    L.trc_group_reduce_accum.argtypes = [vp, C.c_int]
    L.trc_group_reduce_accum_async.argtypes = [vp, C.c_int]
    L.trc_group_allreduce_mean_accum.argtypes = [vp]
    L.trc_group_compose_samples.argtypes = [vp, C.c_int, u32]
    L.trc_group_compose_samples_async.argtypes = [vp, C.c_int, u32]
    L.trc_shard_seed.argtypes = [u64, u32]
    L.trc_device_pci_bus_id.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.trc_download_composed.argtypes = [vp, vp]
    L.trc_group_finalize.argtypes = [vp]
    L.trc_group_set_collectives.argtypes = [vp, vp, C.c_int, C.c_int]
    L.trc_debug_set.argtypes = [vp, C.c_char_p, C.c_int]
    L.trc_debug_block_costs.argtypes = [vp, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
    L.trc_debug_launch_shape.argtypes = [vp, C.POINTER(abi.LaunchShape)]
    L.trc_debug_primary_replays.argtypes = [vp, C.POINTER(u64)]
    L.trc_denoise_default_params.argtypes = [C.POINTER(abi.DenoiseParams)]
    L.trc_denoise.argtypes = [vp, C.POINTER(abi.DenoiseParams)]
    L.trc_download_denoised.argtypes = [vp, vp]
    L.trc_tonemap_denoised.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.trc_download_gbuffer.argtypes = [vp, vp]
    L.trc_denoise_reset.argtypes = [vp]
    L.trc_denoise_track_motion.argtypes = [vp, C.c_int]
    L.trc_denoise_guide_rays.argtypes = [vp, C.c_int]
    L.trc_download_motion.argtypes = [vp, vp]
    L.trc_download_history_length.argtypes = [vp, vp]
    L.trc_upload_textures.argtypes = [vp, C.POINTER(abi.Image), u32]
    L.trc_upload_triangle_materials.argtypes = [vp, vp, u32]
    L.trc_update_vertices.argtypes = [vp, vp, u32, u32]
    L.trc_debug_refit_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.trc_pose_vertices.argtypes = [vp, C.POINTER(abi.Pose), u32]
    L.trc_download_vertices.argtypes = [vp, vp, u32, u32]
    L.trc_debug_pose_overflows.argtypes = [vp, C.POINTER(u32)]
    L.trc_skin_bind.argtypes = [vp, vp, u32, u32]
    L.trc_skin_vertices.argtypes = [vp, C.POINTER(abi.SkinBone), u32]
    L.trc_morph_bind.argtypes = [vp, vp, u32, u32, u32]
    L.trc_morph_vertices.argtypes = [vp, vp, u32, C.POINTER(abi.SkinBone), u32]
    L.trc_recompute_normals.argtypes = [vp, u32, u32]
    L.trc_rebuild_tree.argtypes = [vp, u32]
    L.trc_tree_cost.argtypes = [vp, C.POINTER(abi.TreeCost)]
    L.trc_set_triangle_visibility.argtypes = [vp, C.POINTER(abi.TriangleRange), u32, u32]
    L.trc_download_triangle_visibility.argtypes = [vp, vp]
    L.trc_debug_visibility_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.trc_update_primitives.argtypes = [vp, C.POINTER(abi.PrimitiveRanges)]
    L.trc_set_tile_mask.argtypes = [vp, vp, u32]
    L.trc_download_tile_mask.argtypes = [vp, vp]
    L.trc_tile_snapshot.argtypes = [vp]
    L.trc_tile_error.argtypes = [vp, C.c_int]
    L.trc_download_tile_error.argtypes = [vp, vp]
    L.trc_adaptive_default_params.argtypes = [C.POINTER(abi.AdaptiveParams)]
    L.trc_render_adaptive.argtypes = [vp, C.POINTER(abi.Params), C.POINTER(abi.AdaptiveParams), C.POINTER(abi.AdaptiveReport)]
    L.trc_download_tile_samples.argtypes = [vp, vp]
    L.trc_upload_camera_rays.argtypes = [vp, vp, u32]
    L.trc_generate_camera_rays.argtypes = [vp, C.POINTER(abi.RayGen)]
    L.trc_download_camera_rays.argtypes = [vp, u32, vp]
    L.trc_clear_camera_rays.argtypes = [vp]
    L.trc_upload_material_params.argtypes = [vp, vp, u32]
    L.trc_download_material_params.argtypes = [vp, vp, u32]
    if hooks:
        L.trc_debug_last_camera_rays.argtypes = [vp, C.POINTER(u32)]
        L.trc_debug_last_material_params.argtypes = [vp, C.POINTER(u32)]
        L.trc_material_params_test.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_float, vp]
        L.trc_debug_profile.argtypes = [vp, C.POINTER(C.c_uint64), u32]
        L.trc_sppm_hash_cells.argtypes = [vp, vp, C.c_size_t, C.c_float, vp]
        L.trc_div_by_test.argtypes = [vp, vp, vp, C.c_size_t, vp, vp]
        L.trc_unary_test.argtypes = [vp, u32, u32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(u32)]
        L.trc_debug_denoise_state.argtypes = [vp, vp, vp, vp]
        L.trc_texture_sample_test.argtypes = [vp, u32, vp, C.c_size_t, vp]
        L.trc_debug_env_tables.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_float)]
        L.trc_env_light_test.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp]
        L.trc_debug_mesh_light_tables.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(u32)]
        L.trc_mesh_light_test.argtypes = [vp, vp, vp, C.c_size_t, vp, vp]
        L.trc_debug_last_kernel.argtypes = [vp, C.POINTER(abi.KernelChoice)]
        L.trc_debug_last_residency.argtypes = [vp, C.POINTER(abi.Residency)]
        L.trc_material_s_f_test.argtypes = [vp, u32, vp, vp, vp, vp, C.c_size_t, C.c_float, vp]
        L.trc_sample11_test.argtypes = [vp, u32, vp, C.c_float, u32, vp, C.c_size_t, vp, vp]
        for name in abi.HOOK_SYMBOLS:
            getattr(L, name).restype = i32
    L.trc_has_test_hooks.restype = C.c_int
    for name in abi.DEVICE_SYMBOLS:
        f = getattr(L, name)
        if name not in ("trc_abi_version", "trc_build_flavor", "trc_has_test_hooks", "trc_status_string", "trc_last_error", "trc_destroy", "trc_shard_seed",
                        "trc_denoise_default_params", "trc_adaptive_default_params"):
            f.restype = i32
    L.trc_shard_seed.restype = u64
    L.trc_denoise_default_params.restype = None
    L.trc_adaptive_default_params.restype = None
    if L.trc_abi_version() != abi.TRC_ABI_VERSION:
        raise RuntimeError("libtracer_amd.so ABI version mismatch")
    return L


def make_poses(poses):
    """ctypes array of abi.Pose from a sequence of (first, count, model, normal); the matrices are (4, 4), model[r][c] row r column c"""
    arr = (abi.Pose * len(poses))()
    for k, (first, count, model, normal) in enumerate(poses):
        arr[k].first, arr[k].count = int(first), int(count)
        for name, m in (("model_matrix", model), ("normal_matrix", normal)):
            m = np.asarray(m, dtype=np.float32).reshape(4, 4)
            cols = getattr(arr[k], name).columns
            for c in range(4):
                cols[c].x, cols[c].y, cols[c].z, cols[c].w = (float(m[r, c]) for r in range(4))
    return arr


def make_bones(palette):
    """ctypes array of abi.SkinBone from a sequence of (model, normal); the matrices are (4, 4), m[r][c] row r column c, as make_poses takes"""
    m = np.asarray(palette, dtype=np.float32).reshape(-1, 2, 4, 4)
    cols = np.ascontiguousarray(m.transpose(0, 1, 3, 2))      # stored column-major: [bone, matrix, column, row]
    return (abi.SkinBone * len(cols)).from_buffer_copy(cols.tobytes())


def group_unique_id():
    buf = (C.c_uint8 * abi.TRC_UNIQUE_ID_BYTES)()
    st = lib().trc_group_unique_id(buf)
    if st != abi.OK:
        raise TracerError("trc_group_unique_id", st)
    return bytes(buf)


class Tracer:
    """One context per GPU (single-threaded, one HIP stream)."""

    def __init__(self, device=0, fast_math=False, hooks=False):
        self._L = lib(fast_math, hooks)
        self._env_shape = (0, 0)         # (h, w) of the environment map set through this object
        self._h = C.c_void_p()
        st = self._L.trc_create(device, C.byref(self._h))
        if st != abi.OK:
            self._h = None
            raise TracerError(f"trc_create(device={device})", st, self._L.trc_status_string(st).decode())
        self.width = self.height = 0
        self._n_vertex = 0               # of the scene uploaded through this object (download_vertices' default count)
        self._n_triangle = 0             # ... and its triangles (triangle_visibility's length)

    def _check(self, st, what):
        if st != abi.OK:
            raise TracerError(what, st, self._L.trc_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.trc_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # --- scene / camera / frame -------------------------------------------------
    def upload_scene(self, scene_view):
        self._check(self._L.trc_upload_scene(self._h, C.byref(scene_view)), "trc_upload_scene")
        self._n_vertex = scene_view.n_vertex
        self._n_triangle = scene_view.n_index // 3

    def set_environment_map(self, rgb):
        """(h, w, 3) float32 equirectangular environment; None returns to the constant one."""
        if rgb is None:
            self._check(self._L.trc_set_environment_map(self._h, 0, 0, None), "trc_set_environment_map")
            self._env_shape = (0, 0)
            return
        assert rgb.dtype == np.float32 and rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.flags.c_contiguous
        self._check(self._L.trc_set_environment_map(self._h, rgb.shape[1], rgb.shape[0], rgb.ctypes.data),
                    "trc_set_environment_map")
        self._env_shape = rgb.shape[:2]

    def upload_textures(self, images):
        """Image textures: a list of (h, w, 3) float32 arrays, rows bottom-up (what host.load_png returns); a material with
        textureInfo.type == TEX_IMAGE samples image textureInfo.textureIndex.  An empty list (or None) clears them."""
        images = [np.ascontiguousarray(a, dtype=np.float32) for a in (images or [])]
        for a in images:
            assert a.ndim == 3 and a.shape[2] == 3, a.shape
        arr = (abi.Image * max(1, len(images)))()
        for k, a in enumerate(images):
            arr[k].width, arr[k].height = a.shape[1], a.shape[0]
            arr[k].rgb = a.ctypes.data_as(C.POINTER(C.c_float))
        self._check(self._L.trc_upload_textures(self._h, arr if images else None, len(images)), "trc_upload_textures")

    def upload_triangle_materials(self, material):
        """Per-triangle materials (trc_upload_triangle_materials): one uint32 material index per triangle of the uploaded scene, in
        index-list order; None restores material 19 on every triangle."""
        if material is None:
            self._check(self._L.trc_upload_triangle_materials(self._h, None, 0), "trc_upload_triangle_materials")
            return
        m = np.ascontiguousarray(material, dtype=np.uint32).ravel()
        # an empty array is an array of the wrong length for a scene with triangles (refused), not None: never pass it as NULL
        buf = m if m.size else np.zeros(1, np.uint32)
        self._check(self._L.trc_upload_triangle_materials(self._h, buf.ctypes.data, m.size), "trc_upload_triangle_materials")

    def update_vertices(self, vertices, first=0):
        """trc_update_vertices: (n, 8) float32 rows of trc_TriangleVertex (position, normal, uv) replace vertices [first, first + n) of
        the uploaded scene's triList, and the tree is refitted in place.  The accumulator is not cleared."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 8)
        buf = v if v.size else np.zeros((1, 8), np.float32)      # an empty array is count == 0, never NULL with a count
        self._check(self._L.trc_update_vertices(self._h, buf.ctypes.data, first, v.shape[0]), "trc_update_vertices")

    def pose_vertices(self, poses):
        """trc_pose_vertices: `poses` is a ctypes array of abi.Pose, or a sequence of (first, count, model, normal) with the matrices
        as (4, 4) arrays in the usual row-major mathematical layout (model[r][c]; stored column-major, as simd does).  Every range is
        posed from the scene's REST vertices on the device, and the tree is refitted in place.  The accumulator is not cleared."""
        if not (isinstance(poses, C.Array) and poses._type_ is abi.Pose):
            poses = make_poses(poses)
        self._check(self._L.trc_pose_vertices(self._h, poses if len(poses) else None, len(poses)), "trc_pose_vertices")

    def update_primitives(self, spheres=None, first_sphere=0, squares=None, first_square=0, cubes=None, first_cube=0):
        """trc_update_primitives: each list is a ctypes array (or a sequence) of abi.Sphere / abi.Square / abi.Cube records, or None;
        list k replaces the scene's records [first_k, first_k + len) of its kind, and the tree is refitted in place once.  The
        accumulator is not cleared."""
        r = abi.PrimitiveRanges()
        keep = []
        for name, typ, items, first in (("sphere", abi.Sphere, spheres, first_sphere), ("square", abi.Square, squares, first_square),
                                        ("cube", abi.Cube, cubes, first_cube)):
            n = len(items) if items is not None else 0
            if n and not (isinstance(items, C.Array) and items._type_ is typ):
                items = (typ * n)(*items)
            keep.append(items)
            if n:
                setattr(r, name + "s", C.cast(items, C.POINTER(typ)))
            setattr(r, "first_" + name, int(first))
            setattr(r, "n_" + name, n)
        self._check(self._L.trc_update_primitives(self._h, C.byref(r)), "trc_update_primitives")

    def download_vertices(self, first=0, count=None):
        """trc_download_vertices: the current vertices [first, first + count) on the device as (count, 8) float32 rows (position,
        normal, uv); count None: up to the end of the scene's vertex list."""
        if count is None:
            count = max(self._n_vertex - first, 0)
        out = np.empty((max(count, 0), 8), dtype=np.float32)
        buf = out if out.size else np.zeros((1, 8), np.float32)
        self._check(self._L.trc_download_vertices(self._h, buf.ctypes.data, first, count), "trc_download_vertices")
        return out

    def skin_bind(self, bones, weights, first=0):
        """trc_skin_bind: vertex first + i gets the four influences (bones[i, k], weights[i, k]); `bones` is (n, 4) integers, `weights`
        (n, 4) float32.  One binding per scene: a second call replaces it, an empty array removes it.  Moves no vertex."""
        b = np.asarray(bones, dtype=np.int64).reshape(-1, 4)
        w = np.asarray(weights, dtype=np.float32).reshape(-1, 4)
        if len(b) != len(w):
            raise ValueError(f"skin_bind: {len(b)} rows of bones, {len(w)} rows of weights")
        table = np.empty((len(b), 8), dtype=np.uint32)            # abi.SkinInfluence rows
        table[:, :4] = np.where((b < 0) | (b > 0xFFFFFFFF), 0xFFFFFFFF, b)      # what no uint32 holds is refused by the library
        table[:, 4:] = w.view(np.uint32)
        self._check(self._L.trc_skin_bind(self._h, table.ctypes.data if len(table) else None, first, len(table)), "trc_skin_bind")

    def skin_vertices(self, palette):
        """trc_skin_vertices: `palette` is a ctypes array of abi.SkinBone, or a sequence of (model, normal) with the matrices as (4, 4)
        arrays in the layout make_poses takes.  Every bound vertex (skin_bind) is computed from the scene's REST vertices on the
        device under the blend of its four bones, and the tree is refitted in place.  The accumulator is not cleared."""
        if not (isinstance(palette, C.Array) and palette._type_ is abi.SkinBone):
            palette = make_bones(palette)
        self._check(self._L.trc_skin_vertices(self._h, palette if len(palette) else None, len(palette)), "trc_skin_vertices")

    def morph_bind(self, deltas, first=0):
        """trc_morph_bind: `deltas` is (n_targets, count, 6) float32 -- deltas[k, i] is target k's (dx, dy, dz, dnx, dny, dnz) for
        vertex first + i.  One morph binding per scene: a second call replaces it, an empty array removes it.  Moves no vertex."""
        d = np.ascontiguousarray(deltas, dtype=np.float32)
        if d.ndim != 3 or d.shape[2] != 6:
            raise ValueError(f"morph_bind: deltas of shape {d.shape}, not (n_targets, count, 6)")
        self._check(self._L.trc_morph_bind(self._h, d.ctypes.data if d.size else None, d.shape[0], first, d.shape[1]), "trc_morph_bind")

    def morph_vertices(self, weights, bones=None):
        """trc_morph_vertices: every vertex of the morph binding becomes its REST vertex plus the weighted deltas of the targets whose
        weight is not zero, in ascending order of the target.  `bones` (what skin_vertices takes) puts the skin of skin_bind on top of
        the morphed values in the same call.  The tree is refitted in place; the accumulator is not cleared."""
        w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        buf = w if w.size else np.zeros(1, np.float32)            # an empty array is n_weights == 0, never NULL
        if bones is None or len(bones) == 0:
            bones, n_bones = None, 0
        else:
            if not (isinstance(bones, C.Array) and bones._type_ is abi.SkinBone):
                bones = make_bones(bones)
            n_bones = len(bones)
        self._check(self._L.trc_morph_vertices(self._h, buf.ctypes.data, w.size, bones, n_bones), "trc_morph_vertices")

    def recompute_normals(self, first=0, count=None):
        """trc_recompute_normals: the normals of the current vertices [first, first + count) become area-weighted smooth normals of the
        mesh as it now stands, computed on the device; count None: up to the end of the scene's vertex list.  No position moves and the
        rest copy is not written: call it after each update, pose, skin or morph.  The accumulator is not cleared."""
        if count is None:
            count = max(self._n_vertex - first, 0)
        self._check(self._L.trc_recompute_normals(self._h, first, count), "trc_recompute_normals")

    def pose_overflows(self):
        """posed positions of the last pose_vertices, skinned positions of the last skin_vertices or final positions of the last
        morph_vertices (whichever call came last) that came out non-finite or beyond 1e37 (trc_debug_pose_overflows)"""
        n = C.c_uint32(0)
        self._check(self._L.trc_debug_pose_overflows(self._h, C.byref(n)), "trc_debug_pose_overflows")
        return n.value

    def refit_ms(self):
        """device time in ms of the kernels of the last update_vertices, pose_vertices, skin_vertices, morph_vertices or recompute_normals
        (trc_debug_refit_ms)"""
        ms = C.c_float(0)
        self._check(self._L.trc_debug_refit_ms(self._h, C.byref(ms)), "trc_debug_refit_ms")
        return ms.value

    def texture_sample(self, index, uv):
        """hooks build only: the render kernels' lookup of image `index` at (n, 2) float32 uv -> (n, 3) float32."""
        uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        out = np.empty((uv.shape[0], 3), dtype=np.float32)
        self._check(self._L.trc_texture_sample_test(self._h, index, uv.ctypes.data, uv.shape[0], out.ctypes.data), "trc_texture_sample_test")
        return out

    def env_tables(self):
        """hooks build only: the sampling tables of TRC_FLAG_ENV_LIGHT for the current map -> dict of weight (H, W) float32,
        rows (H, W, 2) uint32 {threshold, alias}, marg (H, 2) uint32, total (float), build_ms (float)."""
        H, W = self._env_shape
        weight = np.empty((H, W), np.float32)
        rows = np.empty((H, W, 2), np.uint32)
        marg = np.empty((H, 2), np.uint32)
        total, ms = C.c_double(), C.c_float()
        self._check(self._L.trc_debug_env_tables(self._h, weight.ctypes.data, rows.ctypes.data, marg.ctypes.data, C.byref(total), C.byref(ms)),
                    "trc_debug_env_tables")
        return dict(weight=weight, rows=rows, marg=marg, total=total.value, build_ms=ms.value)

    def env_light_test(self, draws=None, dirs=None):
        """hooks build only: the render kernels' environment-light sampler on (n, 6) uint32 draws (row index, row alias, cell index,
        cell alias, then two float32 bit patterns) -> (n, 4) float32 direction + pdf, and its pdf of (m, 3) float32 directions -> (m,)"""
        d = np.ascontiguousarray(np.zeros((0, 6), np.uint32) if draws is None else draws, dtype=np.uint32).reshape(-1, 6)
        v = np.ascontiguousarray(np.zeros((0, 3), np.float32) if dirs is None else dirs, dtype=np.float32).reshape(-1, 3)
        out = np.empty((d.shape[0], 4), np.float32)
        pdf = np.empty(v.shape[0], np.float32)
        self._check(self._L.trc_env_light_test(self._h, d.ctypes.data, d.shape[0], out.ctypes.data, v.ctypes.data, v.shape[0], pdf.ctypes.data),
                    "trc_env_light_test")
        return out, pdf

    def mesh_light_tables(self, n_triangles):
        """hooks build only: the sampling tables of TRC_FLAG_MESH_LIGHTS for the uploaded scene (of n_triangles triangles) -> dict of
        alias (n_lights, 2) uint32 {threshold, alias}, tri (n_lights,) uint32, pdfA (n_triangles,) float32, total (float), n_lights."""
        total, n = C.c_double(), C.c_uint32()
        self._check(self._L.trc_debug_mesh_light_tables(self._h, None, None, None, C.byref(total), C.byref(n)), "trc_debug_mesh_light_tables")
        alias = np.zeros((n.value, 2), np.uint32)
        tri = np.zeros(n.value, np.uint32)
        pdfA = np.zeros(n_triangles, np.float32)
        self._check(self._L.trc_debug_mesh_light_tables(self._h, alias.ctypes.data if n.value else None, tri.ctypes.data if n.value else None,
                                                        pdfA.ctypes.data if n_triangles else None, C.byref(total), C.byref(n)),
                    "trc_debug_mesh_light_tables")
        return dict(alias=alias, tri=tri, pdfA=pdfA, total=total.value, n_lights=n.value)

    def mesh_light_test(self, draws, pos):
        """hooks build only: the render kernels' mesh-light sampler on (n, 4) uint32 draws (light index, alias decision, then two
        float32 bit patterns) seen from (n, 3) float32 shading points -> (tri (n,) uint32, out (n, 7) float32: point, normal, pdfA)"""
        d = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1, 4)
        v = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        assert d.shape[0] == v.shape[0]
        tri = np.empty(d.shape[0], np.uint32)
        out = np.empty((d.shape[0], 7), np.float32)
        self._check(self._L.trc_mesh_light_test(self._h, d.ctypes.data, v.ctypes.data, d.shape[0], tri.ctypes.data, out.ctypes.data),
                    "trc_mesh_light_test")
        return tri, out

    def tonemap(self):
        """fragmentShader's auto-exposure + ACES on the accumulator -> ((H, W, 4) uint8, rows top-down; exposure)."""
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        e = C.c_float(0)
        self._check(self._L.trc_tonemap(self._h, out.ctypes.data, C.byref(e)), "trc_tonemap")
        return out, e.value

    def upload_density(self, info, density):
        """Density grid (nz, ny, nx) float32 of the GridDensity medium for integrator 2; None clears it."""
        if density is None:
            self._check(self._L.trc_upload_density(self._h, None, None), "trc_upload_density")
            return
        assert density.dtype == np.float32 and density.flags.c_contiguous
        self._check(self._L.trc_upload_density(self._h, C.byref(info), density.ctypes.data), "trc_upload_density")

    def upload_scene_lbvh(self, leaves_view):
        """Scene whose bvhList holds only leaf records (HostScene.leaves_view()); the tree is built on the GPU."""
        self._check(self._L.trc_upload_scene_lbvh(self._h, C.byref(leaves_view)), "trc_upload_scene_lbvh")
        self._n_vertex = leaves_view.n_vertex
        self._n_triangle = leaves_view.n_index // 3

    def upload_scene_sah(self, leaves_view):
        """Same input as upload_scene_lbvh; the reference's binned-SAH tree (BVH::buildTree), built on the GPU."""
        self._check(self._L.trc_upload_scene_sah(self._h, C.byref(leaves_view)), "trc_upload_scene_sah")
        self._n_vertex = leaves_view.n_vertex
        self._n_triangle = leaves_view.n_index // 3

    def upload_scene_device(self, view, flags):
        """trc_upload_scene_device: abi.TREE_SAH | abi.TREE_TRIANGLE_LEAVES (bvhList = the analytic primitives' leaves only); with
        abi.TREE_SAH, abi.TREE_SAH3 asks for the three-axis, 32-bin split (a tree of lower cost that is no longer the reference's)."""
        self._check(self._L.trc_upload_scene_device(self._h, C.byref(view), flags), "trc_upload_scene_device")
        self._n_vertex = view.n_vertex
        self._n_triangle = view.n_index // 3

    def download_bvh(self):
        """The device-built tree in the reference's array layout: ctypes array of abi.BVH (2n-1 records)."""
        n = C.c_uint32(0)
        self._check(self._L.trc_download_bvh(self._h, None, 0, C.byref(n)), "trc_download_bvh")
        out = (abi.BVH * n.value)()
        self._check(self._L.trc_download_bvh(self._h, out, n.value, C.byref(n)), "trc_download_bvh")
        return out

    def rebuild_tree(self, flags=0):
        """trc_rebuild_tree: a fresh tree over the scene's current leaf records, built on the device from what it holds -- abi.TREE_SAH
        for the reference's binned-SAH tree (| abi.TREE_SAH3: the three-axis, 32-bin split), 0 for the LBVH with rotations.  Vertices, materials,
        rest copy and binding stay."""
        self._check(self._L.trc_rebuild_tree(self._h, flags), "trc_rebuild_tree")

    def tree_cost(self):
        """trc_tree_cost -> abi.TreeCost: half areas of the root box, of the interior child slots and of the leaf child slots of the
        tree as it stands, with the two slot counts; (interior + leaf) / root grows as a refitted tree degrades."""
        out = abi.TreeCost()
        self._check(self._L.trc_tree_cost(self._h, C.byref(out)), "trc_tree_cost")
        return out

    def set_triangle_visibility(self, ranges, flags=0):
        """trc_set_triangle_visibility: `ranges` is a sequence of (first, count, visible) triples (or an abi.TriangleRange array, or None
        for a NULL pointer), applied in order to the scene's per-triangle mask; then the tree over the analytic leaves and the visible
        triangles is built on the device -- flags as for rebuild_tree.  Hidden triangles keep vertices, materials and bindings."""
        if ranges is None:
            arr, n = None, 0
        elif isinstance(ranges, C.Array):
            arr, n = ranges, len(ranges)
        else:
            ranges = [tuple(int(v) for v in r) for r in ranges]
            arr, n = (abi.TriangleRange * max(len(ranges), 1))(*ranges), len(ranges)
        self._check(self._L.trc_set_triangle_visibility(self._h, arr, n, flags), "trc_set_triangle_visibility")

    def triangle_visibility(self):
        """trc_download_triangle_visibility -> uint8 array, one per triangle of the index list, 1 = visible"""
        out = np.zeros(self._n_triangle, dtype=np.uint8)
        self._check(self._L.trc_download_triangle_visibility(self._h, out.ctypes.data if out.size else None), "trc_download_triangle_visibility")
        return out

    def visibility_ms(self):
        """trc_debug_visibility_ms: device time of the last set_triangle_visibility's leaf-list stage (mask, partition, leaf records)"""
        ms = C.c_float(0)
        self._check(self._L.trc_debug_visibility_ms(self._h, C.byref(ms)), "trc_debug_visibility_ms")
        return ms.value

    def lbvh_info(self):
        """(n_nodes, depth of the deepest leaf, GPU build time in ms) of the last upload_scene_lbvh."""
        n, h, ms = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
        self._check(self._L.trc_lbvh_info(self._h, C.byref(n), C.byref(h), C.byref(ms)), "trc_lbvh_info")
        return n.value, h.value, ms.value

    def set_camera(self, camera):
        self._check(self._L.trc_set_camera(self._h, C.byref(camera)), "trc_set_camera")

    def set_environment(self, rgb):
        self._check(self._L.trc_set_environment(self._h, (C.c_float * 3)(*rgb)), "trc_set_environment")

    def resize(self, width, height):
        self._check(self._L.trc_resize(self._h, width, height), "trc_resize")
        self.width, self.height = width, height

    def seed(self, seed):
        self._check(self._L.trc_seed(self._h, seed), "trc_seed")

    def upload_rng(self, rng):
        assert rng.dtype == np.uint32 and rng.shape == (self.height, self.width, 4) and rng.flags.c_contiguous
        self._check(self._L.trc_upload_rng(self._h, rng.ctypes.data), "trc_upload_rng")

    def download_rng(self):
        out = np.empty((self.height, self.width, 4), dtype=np.uint32)
        self._check(self._L.trc_download_rng(self._h, out.ctypes.data), "trc_download_rng")
        return out

    def upload_accum(self, accum):
        assert accum.dtype == np.float32 and accum.shape == (self.height, self.width, 4) and accum.flags.c_contiguous
        self._check(self._L.trc_upload_accum(self._h, accum.ctypes.data), "trc_upload_accum")

    def download_accum(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._L.trc_download_accum(self._h, out.ctypes.data), "trc_download_accum")
        return out

    def clear_accum(self):
        self._check(self._L.trc_clear_accum(self._h), "trc_clear_accum")

    # --- the hot path --------------------------------------------------------------
    def render(self, spp=1, max_depth=8, integrator=abi.INTEGRATOR_PATH, frame0=0, tile_rank=0, tile_nranks=1,
               collect_stats=False, view_height=0, fixed_order=False, sobol=False, small_blocks=None, env_light=False,
               mesh_lights=False, camera_rays=False, material_params=False):
        flags = ((abi.FLAG_COLLECT_STATS if collect_stats else 0) | (abi.FLAG_FIXED_ORDER if fixed_order else 0) |
                 (abi.FLAG_SOBOL if sobol else 0) | (abi.FLAG_ENV_LIGHT if env_light else 0) | (abi.FLAG_MESH_LIGHTS if mesh_lights else 0) |
                 (abi.FLAG_CAMERA_RAYS if camera_rays else 0) | (abi.FLAG_MATERIAL_PARAMS if material_params else 0) |
                 (0 if small_blocks is None else (abi.FLAG_SMALL_BLOCKS if small_blocks else abi.FLAG_LARGE_BLOCKS)))
        prm = abi.Params(spp=spp, max_depth=max_depth, integrator=integrator, frame0=frame0, tile_rank=tile_rank,
                         tile_nranks=tile_nranks, flags=flags, view_height=view_height)
        self._check(self._L.trc_render(self._h, C.byref(prm)), "trc_render")

    def synchronize(self):
        self._check(self._L.trc_synchronize(self._h), "trc_synchronize")

    # --- camera-ray sets (include/tracer_abi.h "Camera-ray sets"; render(camera_rays=True)) -------------------------
    def upload_camera_rays(self, rays):
        """trc_upload_camera_rays: a structured array of trc_ray (dtypes.RAY_DTYPE) of shape (n_sets, H, W), or (H, W) for one set"""
        from .dtypes import RAY_DTYPE
        assert rays.dtype == RAY_DTYPE and rays.flags.c_contiguous and rays.shape[-2:] == (self.height, self.width) and rays.ndim in (2, 3)
        self._check(self._L.trc_upload_camera_rays(self._h, rays.ctypes.data, 1 if rays.ndim == 2 else rays.shape[0]), "trc_upload_camera_rays")

    def generate_camera_rays(self, model=abi.RAYS_PINHOLE, n_sets=1, offsets=None):
        """trc_generate_camera_rays: n_sets sets built on the device from the context's camera; offsets: (n_sets, 2) sub-pixel offsets in
        [0, 1) (host.halton_offsets), None = all zero"""
        g = abi.RayGen(model=model, n_sets=n_sets)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.float32)
            assert offsets.shape == (n_sets, 2), offsets.shape
            g.offsets = offsets.ctypes.data_as(C.POINTER(C.c_float))
        self._check(self._L.trc_generate_camera_rays(self._h, C.byref(g)), "trc_generate_camera_rays")

    def download_camera_rays(self, set=0):
        """trc_download_camera_rays -> (H, W) structured array of trc_ray"""
        from .dtypes import RAY_DTYPE
        out = np.zeros((self.height, self.width), dtype=RAY_DTYPE)
        self._check(self._L.trc_download_camera_rays(self._h, set, out.ctypes.data), "trc_download_camera_rays")
        return out

    def clear_camera_rays(self):
        self._check(self._L.trc_clear_camera_rays(self._h), "trc_clear_camera_rays")

    def last_camera_rays(self):
        """hooks build only: whether the last render launch ran a kernel of TRC_FLAG_CAMERA_RAYS (trc_debug_last_camera_rays)"""
        used = C.c_uint32(0)
        self._check(self._L.trc_debug_last_camera_rays(self._h, C.byref(used)), "trc_debug_last_camera_rays")
        return bool(used.value)

    # --- material parameters (include/tracer_abi.h "Material parameters"; render(material_params=True)) -------------
    def upload_material_params(self, params):
        """trc_upload_material_params: a structured array of trc_material_params (dtypes.MATERIAL_PARAMS_DTYPE), one record per material of
        the scene; None: no table in force"""
        from .dtypes import MATERIAL_PARAMS_DTYPE
        if params is None:
            self._check(self._L.trc_upload_material_params(self._h, None, 0), "trc_upload_material_params")
            return
        assert params.dtype == MATERIAL_PARAMS_DTYPE and params.flags.c_contiguous and params.ndim == 1
        self._check(self._L.trc_upload_material_params(self._h, params.ctypes.data, len(params)), "trc_upload_material_params")

    def download_material_params(self, n_material):
        """trc_download_material_params -> (n_material,) structured array of trc_material_params"""
        from .dtypes import MATERIAL_PARAMS_DTYPE
        out = np.zeros(n_material, dtype=MATERIAL_PARAMS_DTYPE)
        self._check(self._L.trc_download_material_params(self._h, out.ctypes.data, n_material), "trc_download_material_params")
        return out

    def last_material_params(self):
        """hooks build only: whether the last render launch ran a kernel of TRC_FLAG_MATERIAL_PARAMS (trc_debug_last_material_params)"""
        used = C.c_uint32(0)
        self._check(self._L.trc_debug_last_material_params(self._h, C.byref(used)), "trc_debug_last_material_params")
        return bool(used.value)

    def material_params_test(self, op, types, color, params, wo, uu, wi=None, pdf_init=0.0):
        """hooks build only (trc_material_params_test): the kernels' parametrised lobes, one lane per input in this order.  op 0:
        Material::S_F -> (n, 7) float32 wi, f, pdf (an early-out leaves pdf_init in place); op 1: Material::F for (wo, wi) -> (n, 4) f, pdf;
        op 2: op 0 with sample11 evaluating each exp, log and erf_inv once (TRC_SAMPLE11_ONCE 7)"""
        from .dtypes import MATERIAL_PARAMS_DTYPE
        types = np.ascontiguousarray(types, dtype=np.uint32)
        color, wo, uu = (np.ascontiguousarray(a, dtype=np.float32) for a in (color, wo, uu))
        n = len(types)
        assert params.dtype == MATERIAL_PARAMS_DTYPE and params.flags.c_contiguous and params.shape == (n,)
        assert types.ndim == 1 and color.shape == (n, 3) and wo.shape == (n, 3) and uu.shape == (n, 2)
        if op == 1:
            wi = np.ascontiguousarray(wi, dtype=np.float32)
            assert wi.shape == (n, 3)
        out = np.empty((n, 4 if op == 1 else 7), np.float32)
        self._check(self._L.trc_material_params_test(self._h, int(op), types.ctypes.data, color.ctypes.data, params.ctypes.data, wo.ctypes.data,
                                                     wi.ctypes.data if op == 1 else None, uu.ctypes.data, n, float(pdf_init), out.ctypes.data),
                    "trc_material_params_test")
        return out

    # --- tile mask, per-tile error estimate, adaptive sampling (include/tracer_abi.h) ------------------------------
    def tile_grid(self):
        """(tile rows, tile columns) of the frame: TRC_TILE x TRC_TILE tiles, the last row and column partial"""
        return (self.height + abi.TRC_TILE - 1) // abi.TRC_TILE, (self.width + abi.TRC_TILE - 1) // abi.TRC_TILE

    def set_tile_mask(self, mask, n_tiles=None):
        """trc_set_tile_mask: one byte per tile, row-major (any shape that ravels to it); render() then covers the owned tiles with a
        non-zero byte only.  None: every tile again.  n_tiles: what to tell the library instead of the array's length (tests)."""
        if mask is None:
            self._check(self._L.trc_set_tile_mask(self._h, None, 0), "trc_set_tile_mask")
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).ravel()
        buf = m if m.size else np.zeros(1, np.uint8)
        self._check(self._L.trc_set_tile_mask(self._h, buf.ctypes.data, m.size if n_tiles is None else n_tiles), "trc_set_tile_mask")

    def tile_mask(self):
        """trc_download_tile_mask -> (tile rows, tile columns) uint8, 1 = rendered"""
        out = np.zeros(self.tile_grid(), dtype=np.uint8)
        self._check(self._L.trc_download_tile_mask(self._h, out.ctypes.data), "trc_download_tile_mask")
        return out

    def tile_snapshot(self):
        """trc_tile_snapshot: A := the accumulator"""
        self._check(self._L.trc_tile_snapshot(self._h), "trc_tile_snapshot")

    def tile_error(self, snapshot_after=False):
        """trc_tile_error: E_t of every tile of the mask from the accumulator and A; snapshot_after: A := accumulator on those tiles"""
        self._check(self._L.trc_tile_error(self._h, 1 if snapshot_after else 0), "trc_tile_error")

    def tile_errors(self):
        """trc_download_tile_error -> (tile rows, tile columns) float32"""
        out = np.zeros(self.tile_grid(), dtype=np.float32)
        self._check(self._L.trc_download_tile_error(self._h, out.ctypes.data), "trc_download_tile_error")
        return out

    def adaptive_params(self, **overrides):
        """trc_adaptive_default_params, then the named fields replaced"""
        a = abi.AdaptiveParams()
        self._L.trc_adaptive_default_params(C.byref(a))
        for k, v in overrides.items():
            setattr(a, k, v)
        return a

    def render_adaptive(self, threshold=None, max_spp=None, spp=8, max_depth=8, integrator=abi.INTEGRATOR_MIS, frame0=0, tile_rank=0,
                        tile_nranks=1, flags=0, view_height=0):
        """trc_render_adaptive: a first pass of `spp` samples, then passes that double the count on the tiles whose estimate is still
        above `threshold`, up to max_spp (None: the library's defaults) -> abi.AdaptiveReport"""
        a = self.adaptive_params()
        if threshold is not None:
            a.threshold = threshold
        if max_spp is not None:
            a.max_spp = max_spp
        prm = abi.Params(spp=spp, max_depth=max_depth, integrator=integrator, frame0=frame0, tile_rank=tile_rank, tile_nranks=tile_nranks,
                         flags=flags, view_height=view_height)
        rep = abi.AdaptiveReport()
        self._check(self._L.trc_render_adaptive(self._h, C.byref(prm), C.byref(a), C.byref(rep)), "trc_render_adaptive")
        return rep

    def tile_samples(self):
        """trc_download_tile_samples -> (tile rows, tile columns) uint32: n_t of the last render_adaptive"""
        out = np.zeros(self.tile_grid(), dtype=np.uint32)
        self._check(self._L.trc_download_tile_samples(self._h, out.ctypes.data), "trc_download_tile_samples")
        return out

    def trace_rays(self, rays, any_hit=False, production=False):
        """rays: structured array with the layout of trc_ray -> structured array of trc_hit.
        production=True walks the tree as the render kernels do (no counters)."""
        from .dtypes import HIT_DTYPE, RAY_DTYPE
        assert rays.dtype == RAY_DTYPE and rays.flags.c_contiguous
        hits = np.zeros(len(rays), dtype=HIT_DTYPE)
        self._check(self._L.trc_trace_rays(self._h, rays.ctypes.data, len(rays), hits.ctypes.data,
                                           (abi.TRACE_ANY_HIT if any_hit else 0) | (abi.TRACE_PRODUCTION if production else 0)),
                    "trc_trace_rays")
        return hits

    # --- SVGF denoiser (include/tracer_abi.h "SVGF denoiser") ----------------------------------------------------
    def denoise_params(self, **overrides):
        """trc_denoise_default_params, then the named fields replaced (demodulate=True sets TRC_DENOISE_DEMODULATE)."""
        p = abi.DenoiseParams()
        self._L.trc_denoise_default_params(C.byref(p))
        if overrides.pop("demodulate", False):
            p.flags |= abi.DENOISE_DEMODULATE
        for k, v in overrides.items():
            setattr(p, k, v)
        return p

    def denoise(self, params=None, **overrides):
        """trc_denoise on the accumulator as it stands (asynchronous); params: abi.DenoiseParams or field overrides."""
        p = params if params is not None else self.denoise_params(**overrides)
        self._check(self._L.trc_denoise(self._h, C.byref(p)), "trc_denoise")

    def download_denoised(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._L.trc_download_denoised(self._h, out.ctypes.data), "trc_download_denoised")
        return out

    def tonemap_denoised(self):
        """trc_tonemap's output stage on the denoised frame -> ((H, W, 4) uint8, rows top-down; exposure)."""
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        e = C.c_float(0)
        self._check(self._L.trc_tonemap_denoised(self._h, out.ctypes.data, C.byref(e)), "trc_tonemap_denoised")
        return out, e.value

    def download_gbuffer(self):
        """(H, W) structured array of trc_gbuffer_texel (tracer_amd.dtypes.GBUFFER_DTYPE)."""
        from .dtypes import GBUFFER_DTYPE
        out = np.empty((self.height, self.width), dtype=GBUFFER_DTYPE)
        self._check(self._L.trc_download_gbuffer(self._h, out.ctypes.data), "trc_download_gbuffer")
        return out

    def denoise_reset(self):
        self._check(self._L.trc_denoise_reset(self._h), "trc_denoise_reset")

    def denoise_track_motion(self, on=True):
        """trc_denoise_track_motion: the history follows the surfaces that update / pose / skin / morph_vertices move (off by default)."""
        self._check(self._L.trc_denoise_track_motion(self._h, 1 if on else 0), "trc_denoise_track_motion")

    def denoise_guide_rays(self, on=True):
        """trc_denoise_guide_rays: the denoiser's G-buffer is walked along set 0 of the camera-ray sets in force, not along the camera's own ray
        (off by default); a change of the switch drops the history."""
        self._check(self._L.trc_denoise_guide_rays(self._h, 1 if on else 0), "trc_denoise_guide_rays")

    def download_motion(self):
        """(H, W) structured array of trc_motion_texel (tracer_amd.dtypes.MOTION_DTYPE): the plane the last trc_denoise used."""
        from .dtypes import MOTION_DTYPE
        out = np.empty((self.height, self.width), dtype=MOTION_DTYPE)
        self._check(self._L.trc_download_motion(self._h, out.ctypes.data), "trc_download_motion")
        return out

    def download_history_length(self):
        """trc_download_history_length: (H, W) float32, the history length n of every pixel as the last trc_denoise left it."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        self._check(self._L.trc_download_history_length(self._h, out.ctypes.data), "trc_download_history_length")
        return out

    def denoise_state(self):
        """hooks build only: (integrated, history, moments), (H, W, 4) float32 each, as the last trc_denoise left them."""
        planes = [np.empty((self.height, self.width, 4), dtype=np.float32) for _ in range(3)]
        self._check(self._L.trc_debug_denoise_state(self._h, *(p.ctypes.data for p in planes)), "trc_debug_denoise_state")
        return tuple(planes)

    def stats(self):
        s = abi.Stats()
        self._check(self._L.trc_get_stats(self._h, C.byref(s)), "trc_get_stats")
        return s

    PROFILE_SITES = ["loop", "box_step", "square", "sphere", "cube", "triangle", "shade", "lambert", "metal",
                     "beckmann_sample", "beckmann_eval", "path_end"]

    def debug_profile(self):
        """{site: (lanes, wavefronts, lanes/(64*wavefronts), cycles)} of the instrumented kernels."""
        n = len(self.PROFILE_SITES)
        buf = (C.c_uint64 * (3 * n))()
        self._check(self._L.trc_debug_profile(self._h, buf, n), "trc_debug_profile")
        return {s: (buf[3 * i], buf[3 * i + 1], buf[3 * i] / (64.0 * buf[3 * i + 1]) if buf[3 * i + 1] else 0.0,
                    buf[3 * i + 2]) for i, s in enumerate(self.PROFILE_SITES)}

    def reset_stats(self):
        self._check(self._L.trc_reset_stats(self._h), "trc_reset_stats")

    def device_info(self):
        name = C.create_string_buffer(256)
        cu, mem = C.c_int(), C.c_size_t()
        self._check(self._L.trc_device_info(self._h, name, 256, C.byref(cu), C.byref(mem)), "trc_device_info")
        return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}

    # --- SPPM pass (Photon.metal) -----------------------------------------------------
    def sppm_init(self, photon_seed):
        self._check(self._L.trc_sppm_init(self._h, photon_seed), "trc_sppm_init")

    def sppm_frames(self, n_frames=1):
        self._check(self._L.trc_sppm_frames(self._h, n_frames), "trc_sppm_frames")

    def sppm_hash_cells(self, cells, hash_scale):
        """Photon.hh hash() of n cell indices (n x 3 float32) at one scale, evaluated on the device."""
        cells = np.ascontiguousarray(cells, dtype=np.float32).reshape(-1, 3)
        out = np.empty(len(cells), dtype=np.float32)
        self._check(self._L.trc_sppm_hash_cells(self._h, cells.ctypes.data, len(cells), float(hash_scale), out.ctypes.data),
                    "trc_sppm_hash_cells")
        return out

    def sppm_download(self):
        """(camera records, photon records, mark grid, count grid, Complex) in the reference's layouts"""
        from .dtypes import CAMREC_DTYPE, PHOTON_DTYPE
        n = abi.PHOTON_HASHN
        cam = np.zeros(self.width * self.height, dtype=CAMREC_DTYPE)
        pho = np.zeros(n * n, dtype=PHOTON_DTYPE)
        mark = np.zeros((n, n, 4), dtype=np.float32)
        count = np.zeros((n, n), dtype=np.float32)
        cx = abi.Complex()
        self._check(self._L.trc_sppm_download(self._h, cam.ctypes.data, pho.ctypes.data, mark.ctypes.data,
                                              count.ctypes.data, C.byref(cx)), "trc_sppm_download")
        return cam, pho, mark, count, cx

    # --- multi-GPU -------------------------------------------------------------------
    def group_init(self, unique_id, nranks, rank):
        buf = (C.c_uint8 * abi.TRC_UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._L.trc_group_init(self._h, buf, nranks, rank), "trc_group_init")

    def group_reduce_accum(self, root=0):
        self._check(self._L.trc_group_reduce_accum(self._h, root), "trc_group_reduce_accum")

    def group_allreduce_mean_accum(self):
        """Sample sharding composed into EVERY rank's accumulator: rank-ordered sum of the ranks' whole-frame accumulators
        over the number of ranks (trc_group_allreduce_mean_accum)."""
        self._check(self._L.trc_group_allreduce_mean_accum(self._h), "trc_group_allreduce_mean_accum")

    def group_compose_samples(self, root=0, sample_groups=None):
        """Sample sharding (tracer_abi.h): rank-ordered sum of the ranks' accumulators / sample_groups, to `root`
        (download_composed); sample_groups defaults to the number of ranks (no tile split inside a group)."""
        self._check(self._L.trc_group_compose_samples(self._h, root, sample_groups or 0), "trc_group_compose_samples")

    def group_compose_samples_async(self, root=0, sample_groups=None):
        self._check(self._L.trc_group_compose_samples_async(self._h, root, sample_groups or 0), "trc_group_compose_samples_async")

    def pci_bus_id(self):
        buf = C.create_string_buffer(64)
        self._check(self._L.trc_device_pci_bus_id(self._h, buf, 64), "trc_device_pci_bus_id")
        return buf.value.decode()

    def group_reduce_accum_async(self, root=0):
        """Compose on a second stream and switch to the other accumulator (see trc_group_reduce_accum_async)."""
        self._check(self._L.trc_group_reduce_accum_async(self._h, root), "trc_group_reduce_accum_async")

    def download_composed(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._L.trc_download_composed(self._h, out.ctypes.data), "trc_download_composed")
        return out

    def set_collectives(self, table, nranks, rank):
        """Caller-supplied collectives instead of an RCCL communicator (trc_group_set_collectives); `table` is an
        object with a ctypes `table` attribute (tracer_amd.gloo_collectives.GlooCollectives) and must outlive the group."""
        self._coll = table
        self._check(self._L.trc_group_set_collectives(self._h, C.byref(table.table) if table is not None else None, nranks, rank),
                    "trc_group_set_collectives")

    def debug_set(self, knob, value):
        """A/B and test knobs of this context (trc_debug_set): scheduling only, never a pixel."""
        self._check(self._L.trc_debug_set(self._h, knob.encode(), int(value)), "trc_debug_set")

    def last_kernel(self):
        """hooks build only: which render kernel the last launch took (trc_debug_last_kernel) -> dict of shape ("one", "strip", "pwg",
        "dense"), variant ("plain", "stats", "sobol", "tex", "env", "env_tex", "mesh", "mesh_tex"), lds_resident, triangle_materials
        (bools), strip (blocks per wavefront) and launches (kernel choices since the context was made)."""
        k = abi.KernelChoice()
        self._check(self._L.trc_debug_last_kernel(self._h, C.byref(k)), "trc_debug_last_kernel")
        return dict(shape=abi.KERNEL_SHAPES[k.shape], variant=abi.KERNEL_VARIANTS[k.variant], lds_resident=bool(k.lds_resident),
                    triangle_materials=bool(k.triangle_materials), strip=int(k.strip), launches=int(k.launches))

    def last_residency(self):
        """hooks build only: how the kernel of the last launch sits on a CU (trc_debug_last_residency) -> dict of cu_count, block (threads
        per workgroup), waves (per SIMD, the kernel's launch bounds), planned_per_cu (workgroups per CU the plan is for), planned_with
        (the runtime's answer the planner used), per_cu (the runtime's answer now) and lds_bytes (dynamic LDS per workgroup)."""
        r = abi.Residency()
        self._check(self._L.trc_debug_last_residency(self._h, C.byref(r)), "trc_debug_last_residency")
        return {name: int(getattr(r, name)) for name, _ in abi.Residency._fields_}

    def material_s_f_test(self, types, color, wo, uu, stream, pdf_init=0.0):
        """(n, 7) float32: wi, attenuation, pdf of the kernels' material_S_F, one lane per input in this order; stream: the Metal lobe
        through the Beckmann lobes' stream (TRC_MICROFACET_STREAM) or as a branch of its own; 2 and 3: those two with sample11 evaluating
        each exp, log and erf_inv once (TRC_SAMPLE11_ONCE 7).  An early-out leaves pdf_init in place."""
        types = np.ascontiguousarray(types, dtype=np.uint32)
        color, wo, uu = (np.ascontiguousarray(a, dtype=np.float32) for a in (color, wo, uu))
        n = len(types)
        assert types.ndim == 1 and color.shape == (n, 3) and wo.shape == (n, 3) and uu.shape == (n, 2)
        out = np.empty((n, 7), np.float32)
        self._check(self._L.trc_material_s_f_test(self._h, int(stream), types.ctypes.data, color.ctypes.data, wo.ctypes.data,
                                                  uu.ctypes.data, n, float(pdf_init), out.ctypes.data), "trc_material_s_f_test")
        return out

    def sample11_test(self, form, family, alpha_y, cap, cos_theta, sin_theta, u1, u2):
        """(slopes (n, 2) float32, exit kinds (n,) uint32) of the kernels' sample11 alone, one lane per input in this order
        (trc_sample11_test).  form: 0 a branch per family, 1 the stream, 2 and 3 those with TRC_SAMPLE11_ONCE 7; family: 0 Beckmann, 1
        Trowbridge-Reitz per input; cap: the Newton loop's bound (10, 3 or 2)."""
        family = np.ascontiguousarray(family, dtype=np.uint32)
        n = len(family)
        packed = np.ascontiguousarray(np.stack([np.asarray(a, np.float32) for a in (cos_theta, sin_theta, u1, u2)], axis=1))
        assert family.ndim == 1 and packed.shape == (n, 4)
        slopes, kind = np.empty((n, 2), np.float32), np.empty(n, np.uint32)
        self._check(self._L.trc_sample11_test(self._h, int(form), family.ctypes.data, float(alpha_y), int(cap), packed.ctypes.data, n,
                                              slopes.ctypes.data, kind.ctypes.data), "trc_sample11_test")
        return slopes, kind

    def div_by_test(self, a, b):
        """(fast, plain): 3 quotients per operand pair through the guarded shared-divisor division and through `/`."""
        a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
        assert a.shape == b.shape and a.ndim == 1
        fast, plain = np.empty((len(a), 3), np.float32), np.empty((len(a), 3), np.float32)
        self._check(self._L.trc_div_by_test(self._h, a.ctypes.data, b.ctypes.data, len(a), fast.ctypes.data, plain.ctypes.data), "trc_div_by_test")
        return fast, plain

    def block_costs(self):
        """(tiles, costs, blk_shift) of the last render launch (trc_debug_block_costs)."""
        n, bs = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.trc_debug_block_costs(self._h, None, None, 0, C.byref(n), C.byref(bs)), "trc_debug_block_costs")
        tiles, costs = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        self._check(self._L.trc_debug_block_costs(self._h, tiles.ctypes.data, costs.ctypes.data, n.value, C.byref(n), C.byref(bs)),
                    "trc_debug_block_costs")
        return tiles, costs, bs.value

    def unary_test(self, op, first_bits=0, count=1 << 32):
        """(mismatches, first mismatching bit pattern) of rcp_cr / sqrt_cr / rsqrt_cr (op 0 / 1 / 2) and the constant-divisor quotients (op 3 .. 6) against the compiler's sequences"""
        n, first = C.c_uint64(0), C.c_uint32(0)
        self._check(self._L.trc_unary_test(self._h, op, first_bits, count, C.byref(n), C.byref(first)), "trc_unary_test")
        return n.value, first.value

    def launch_shape(self):
        """chain bound / work bound of the last render launch (trc_debug_launch_shape) as a dict"""
        s = abi.LaunchShape()
        self._check(self._L.trc_debug_launch_shape(self._h, C.byref(s)), "trc_debug_launch_shape")
        return {k: getattr(s, k) for k, _ in abi.LaunchShape._fields_}

    def primary_replays(self):
        """camera rays answered from the memo of the pixel's first walk since the last reset_stats (trc_debug_primary_replays)"""
        n = C.c_uint64(0)
        self._check(self._L.trc_debug_primary_replays(self._h, C.byref(n)), "trc_debug_primary_replays")
        return n.value

    def group_finalize(self):
        self._check(self._L.trc_group_finalize(self._h), "trc_group_finalize")
