"""examples/trc_render --hide FIRST:COUNT: trc_set_triangle_visibility through the C ABI only, against the Python path fed the same mesh
and the same ranges -- the tonemapped frame, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tracer_amd import abi, host

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "examples", "trc_render")
OBJ = "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nv 1 1 1\nf 1 3 2\nf 1 2 4\nf 2 3 4\nf 1 4 3\nf 2 5 3\nf 3 5 4\nf 4 5 2\n"


@pytest.mark.parametrize("device_sah", [False, True], ids=["host_tree", "device_sah"])
def test_example_hides_what_the_python_path_hides(gpu, tmp_path, device_sah):
    from PIL import Image
    W, H, spp = 96, 64, 4
    obj, out = tmp_path / "solid.obj", tmp_path / "frame.png"
    obj.write_text(OBJ)
    args = [EXE, "--mesh", str(obj), "--size", str(W), str(H), "--spp", str(spp), "--hide", "1:3", "--hide", "5:1", "--out", str(out)]
    log = subprocess.check_output(args + (["--device-sah"] if device_sah else []), text=True, timeout=120)
    print(log)
    got = np.asarray(Image.open(out).convert("RGBA"))
    mesh = host.Mesh.load_obj(str(obj))
    assert mesh.n_triangles == 7
    sc = host.HostScene(abi.SCENE_CORNELL_MESH, mesh, analytic_leaves_only=device_sah)      # (kept alive: the view points into it)
    if device_sah:
        gpu.upload_scene_device(sc.view, abi.TREE_SAH | abi.TREE_TRIANGLE_LEAVES)
    else:
        gpu.upload_scene(sc.view)

    def tonemapped():
        gpu.set_camera(host.prepare_camera(W, H)); gpu.set_environment((0.0, 0.0, 0.0)); gpu.resize(W, H)
        gpu.seed(0x5EED0000); gpu.clear_accum()
        gpu.render(spp=spp, integrator=abi.INTEGRATOR_PATH)
        return gpu.tonemap()[0]

    whole = tonemapped()
    n_before = gpu.tree_cost().n_leaves
    gpu.set_triangle_visibility([(1, 3, 0), (5, 1, 0)], abi.TREE_SAH)
    assert gpu.triangle_visibility().tolist() == [1, 0, 0, 0, 1, 0, 1]
    assert f"a tree of {n_before - 4} leaves" in log
    want = tonemapped()
    assert got.shape == want.shape and (got == want).all() and not (want == whole).all()
    bad = subprocess.run([EXE, "--hide", "3"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--hide" in bad.stderr
