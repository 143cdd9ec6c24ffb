"""examples/trc_render --denoise: an animating C++ host that keeps the SVGF history (trc_denoise_track_motion) through the C ABI only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "trc_render")


def write_ball_obj(path, n_lat=10, n_lon=16):
    """a unit sphere as a Wavefront OBJ with its normals"""
    lines, grid = [], {}
    for a in range(n_lat + 1):
        for b in range(n_lon):
            t, p = np.pi * a / n_lat, 2.0 * np.pi * b / n_lon
            x, y, z = np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)
            grid[a, b] = len(grid) + 1
            lines.append(f"v {x:.6f} {y:.6f} {z:.6f}\nvn {x:.6f} {y:.6f} {z:.6f}")
    for a in range(n_lat):
        for b in range(n_lon):
            q = [grid[a, b], grid[a + 1, b], grid[a + 1, (b + 1) % n_lon], grid[a, (b + 1) % n_lon]]
            if a > 0:
                lines.append("f " + " ".join(f"{k}//{k}" for k in (q[0], q[1], q[3])))
            if a < n_lat - 1:
                lines.append("f " + " ".join(f"{k}//{k}" for k in (q[1], q[2], q[3])))
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["--pose", "--spin", "--bend", "--morph"])
def test_denoise_keeps_the_history_across_the_animation(tmp_path, flag):
    from PIL import Image
    W, H, n = 96, 64, 4
    out = tmp_path / "frame.png"
    write_ball_obj(tmp_path / "ball.obj")
    args = [EXE, "--mesh", str(tmp_path / "ball.obj"), "--size", str(W), str(H), "--spp", "1", flag, "8", "--out", str(out)]
    log = subprocess.run(args + ["--denoise"], text=True, capture_output=True, timeout=120)
    assert log.returncode == 0, log.stderr
    lengths = [float(x) for x in re.findall(r"mean history length ([0-9.]+)", log.stdout)]
    assert len(lengths) == 9 and lengths[0] == 1.0, log.stdout
    # the walls are most of the frame: the mean grows by nearly one per frame although the mesh makes an eighth of a turn each time
    assert all(b > a + 0.5 for a, b in zip(lengths[:n], lengths[1:n + 1])), lengths
    img = np.asarray(Image.open(str(out) + ".3.png").convert("RGBA"))
    assert img.shape == (H, W, 4) and img[..., :3].any()
    # without the flag the same command line is what it was: no denoiser, no history line
    plain = subprocess.run(args, text=True, capture_output=True, timeout=120)
    assert plain.returncode == 0 and "mean history length" not in plain.stdout and "denoised" not in plain.stdout
