"""examples/trc_render --aa / --projection: a C++ host that generates camera-ray sets on the device (trc_generate_camera_rays, Halton offsets
from trc_host_halton_offsets) and renders with TRC_FLAG_CAMERA_RAYS -- through the C ABI only."""
import os
import re
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
def test_aa_renders_through_halton_offset_ray_sets(tmp_path):
    text, frame = _run(tmp_path, "--aa", "4")
    m = re.search(r"camera rays: (\d+) sets, pinhole with Halton offsets, (\S+) MB", text)
    assert m and int(m.group(1)) == 4 and abs(float(m.group(2)) - 4 * W * H * 32 / 1e6) < 0.06, text
    assert f" {W}x{H} 16 spp path:" in text
    plain, frame0 = _run(tmp_path)                         # without the option the command line is what it was
    assert "camera rays:" not in plain
    assert (frame != frame0).any()                           # sub-pixel offsets: another picture of the same scene


@pytest.mark.gpu
def test_equirect_projection_renders_a_panorama(tmp_path):
    text, frame = _run(tmp_path, "--projection", "equirect", "--integrator", "mis")
    assert re.search(r"camera rays: 1 set, equirectangular, ", text) and f" {W}x{H} 16 spp mis:" in text, text


def test_bad_options_are_refused_before_anything_runs():
    for args in (["--aa", "0"], ["--aa", "1025"], ["--projection", "fisheye"]):
        r = subprocess.run([EXE, *args], text=True, capture_output=True, timeout=60)
        assert r.returncode == 2 and "wants" in r.stderr, (args, r.stderr)
