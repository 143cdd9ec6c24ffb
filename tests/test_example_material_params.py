"""examples/trc_render --material-params: a C++ host that builds a table of trc_host_default_material_params, changes the entries the
command line names and renders with TRC_FLAG_MATERIAL_PARAMS -- through the C ABI only."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "trc_render")
W, H = 104, 72


def _run(tmp_path, *extra):
    from PIL import Image
    out = tmp_path / "frame.png"
    log = subprocess.run([EXE, "--scene", "spheres", "--size", str(W), str(H), "--spp", "16", "--out", str(out), *extra], text=True, capture_output=True, timeout=120)
    assert log.returncode == 0, log.stderr
    frame = np.asarray(Image.open(str(out)).convert("RGBA"))
    assert frame.shape == (H, W, 4) and frame[..., :3].any()
    return log.stdout, frame


@pytest.mark.gpu
def test_a_rough_metal_cube_is_another_picture_and_the_literals_are_the_same_one(tmp_path):
    plain, frame0 = _run(tmp_path)                                    # without the option the command line is what it was
    assert "material parameters:" not in plain
    text, same = _run(tmp_path, "--material-params", "0:0.01:0.02")  # material 0 is the Metal cube's: its own literals
    assert "material parameters: 1 of " in text and f" {W}x{H} 16 spp path:" in text, text
    assert np.array_equal(same, frame0)
    text, rough = _run(tmp_path, "--material-params", "0:0.3:0.3", "--material-params", "1:0.01:0.01:1.3", "--integrator", "mis")
    assert "material parameters: 2 of " in text and f" {W}x{H} 16 spp mis:" in text, text
    _, mis0 = _run(tmp_path, "--integrator", "mis")
    assert (rough != mis0).any()


def test_bad_options_are_refused_before_anything_runs():
    for args in (["--material-params", "0:0:0.1"], ["--material-params", "3"], ["--material-params", "1:0.1:0.1:1.0"], ["--material-params", "x:0.1:0.1"]):
        r = subprocess.run([EXE, *args], text=True, capture_output=True, timeout=60)
        assert r.returncode == 2 and "wants" in r.stderr, (args, r.stderr)
