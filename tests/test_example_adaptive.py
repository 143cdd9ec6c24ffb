"""examples/trc_render --adaptive: a C++ host that renders through trc_render_adaptive, prints the report and writes the per-tile sample
counts as a grey image beside the frame -- through the C ABI only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "trc_render")
TILE = 16


@pytest.mark.gpu
def test_adaptive_report_matches_the_per_tile_image(tmp_path):
    from PIL import Image
    W, H, h0, max_spp = 104, 72, 8, 64                       # 7 x 5 tiles, the last column 8 wide, the last row 8 high
    out = tmp_path / "frame.png"
    args = [EXE, "--scene", "spheres", "--size", str(W), str(H), "--spp", str(h0), "--out", str(out)]
    # the threshold: the median estimate that a run which stops nothing reports (a threshold no tile can reach)
    probe = subprocess.run(args + ["--adaptive", "1e-30", "--max-spp", "16"], text=True, capture_output=True, timeout=120)
    assert probe.returncode == 0, probe.stderr
    m = re.search(r"adaptive: .* (\d+) passes, (\d+) samples .* (\d+) of (\d+) tiles still active, error median (\S+) max (\S+) ->", probe.stdout)
    assert m, probe.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) == (2, W * H * 16, 35, 35)
    median = float(m.group(5))
    assert 0 < median <= float(m.group(6))
    log = subprocess.run(args + ["--adaptive", repr(median), "--max-spp", str(max_spp)], text=True, capture_output=True, timeout=120)
    assert log.returncode == 0, log.stderr
    assert " mis:" in log.stdout                             # traceMIS unless --integrator says otherwise
    m = re.search(r"adaptive: threshold (\S+), first pass 8, max 64 spp: (\d+) passes, (\d+) samples .* (\d+) of 35 tiles still active", log.stdout)
    assert m, log.stdout
    passes, samples, active = int(m.group(2)), int(m.group(3)), int(m.group(4))
    grey = np.asarray(Image.open(str(out) + ".samples.png").convert("RGBA"))[..., 0]
    assert grey.shape == (H, W)
    counts = np.array([16, 32, 64])
    n = counts[np.abs(grey[..., None].astype(np.int64) * max_spp - counts * 255).argmin(axis=2)]      # each pixel's tile count
    assert ((255 * n + max_spp // 2) // max_spp == grey).all()
    assert int(n.sum()) == samples and 2 <= passes <= 4 and W * H * 16 < samples < W * H * max_spp
    for ty in range(0, H, TILE):                             # one count per tile, the image's rows top-down
        for tx in range(0, W, TILE):
            rows = slice(max(0, H - ty - TILE), H - ty)
            assert len(np.unique(n[rows, tx:tx + TILE])) == 1
    assert active <= int((n == max_spp).sum() // 1) and (n == 16).any()
    frame = np.asarray(Image.open(str(out)).convert("RGBA"))
    assert frame.shape == (H, W, 4) and frame[..., :3].any()
    # without the flag the same command line is what it was
    plain = subprocess.run(args, text=True, capture_output=True, timeout=120)
    assert plain.returncode == 0 and "adaptive:" not in plain.stdout and " path:" in plain.stdout
