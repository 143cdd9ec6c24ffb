"""Writes tests/golden/pbrt_plain_load.json: sha256 of every array, the camera, the info record and the shape records that
trc_host_scene_load_pbrt returns for the pbrt fixtures of tests/test_pbrt_triangle_materials.py, as recorded with the library of the
commit before per-triangle materials existed (TRC_HOST_LIB=<that build>/tracer_amd/lib/libtrc_host.so python make_pbrt_plain_load.py).
test_pbrt_triangle_materials.py holds the plain load and the flags-0 load of today's library to these digests."""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from test_pbrt_triangle_materials import FIXTURES, digests  # noqa: E402
from tracer_amd import host  # noqa: E402


def plain_lib():
    """the library of TRC_HOST_LIB with just what a plain load uses bound (that library has no trc_host_scene_load_pbrt_flags)"""
    import ctypes as C
    from tracer_amd import abi
    L = C.CDLL(host.lib_path())
    L.trc_host_scene_load_pbrt.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(abi.Camera), C.POINTER(abi.PbrtInfo),
                                           C.POINTER(abi.PbrtShape), C.c_uint32]
    L.trc_host_scene_load_pbrt.restype = C.c_int32
    L.trc_host_scene_view.argtypes = [C.c_void_p, C.POINTER(abi.Scene)]
    L.trc_host_scene_view.restype = None
    L.trc_host_scene_destroy.argtypes = [C.c_void_p]
    L.trc_host_scene_destroy.restype = None
    return L


def main():
    host._LIB = plain_lib()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, text in FIXTURES.items():
            path = os.path.join(d, name + ".pbrt")
            with open(path, "w") as f:
                f.write(text)
            with open(os.path.join(d, "wedge.ply"), "w") as f:
                from test_pbrt_scene import WEDGE_PLY
                f.write(WEDGE_PLY)
            out[name] = digests(*host.HostScene.from_pbrt(path))
    with open(os.path.join(HERE, "pbrt_plain_load.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
