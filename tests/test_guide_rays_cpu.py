"""What TRC_FLAG_CAMERA_RAYS | TRC_FLAG_ENV_LIGHT and trc_denoise_guide_rays need that no device is needed for: the header, the ctypes
mirror and the three built libraries agree on the new entry point; the example host takes its new option combinations.  One run of the
example on the GPU goes with them: a panorama lit by its map, denoised along the rays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tracer_amd import abi, device

HEADER = os.path.join(ROOT, "include", "tracer_abi.h")
EXE = os.path.join(ROOT, "examples", "trc_render")
NAME = "trc_denoise_guide_rays"


def test_header_mirror_and_libraries_agree_on_the_entry_point():
    text = open(HEADER).read()
    assert re.search(r"^trc_status\s+" + NAME + r"\(trc_ctx\* ctx, int on\);", text, re.M)
    assert abi.DEVICE_SYMBOLS.count(NAME) == 1 and NAME not in abi.HOOK_SYMBOLS
    for path in (device.lib_path(), device.fast_lib_path(), device.hooks_lib_path()):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert any(line.split()[-1] == NAME for line in out.splitlines() if line.strip()), path
    for kw in (dict(), dict(fast_math=True), dict(hooks=True)):
        fn = getattr(device.lib(**kw), NAME)
        assert list(fn.argtypes) == [C.c_void_p, C.c_int]
        assert fn(None, 1) == abi.ERR_INVALID_ARG and fn(None, 0) == abi.ERR_INVALID_ARG      # a NULL context, before any device is touched
    assert callable(device.Tracer.denoise_guide_rays)


def test_the_header_states_both_definitions():
    text = open(HEADER).read()
    assert "TRC_FLAG_CAMERA_RAYS | TRC_FLAG_ENV_LIGHT" in text and "A denoiser that follows the rays" in text
    assert re.search(r"added under 13, the number stays: TRC_FLAG_CAMERA_RAYS \| TRC_FLAG_ENV_LIGHT.*?trc_denoise_guide_rays", text, re.S)
    assert abi.TRC_ABI_VERSION == 13


COMBINATIONS = (["--aa", "4", "--env-light", "--integrator", "mis"],
                ["--projection", "equirect", "--env-light", "--integrator", "mis"],
                ["--projection", "ortho", "--aa", "2", "--env-light", "--integrator", "mis", "--denoise"],
                ["--projection", "equirect", "--denoise"])


@pytest.mark.parametrize("args", COMBINATIONS, ids=lambda a: " ".join(a))
def test_example_takes_the_new_option_combinations(tmp_path, args):
    """Parsed, and not refused by the host itself: the run ends where the first thing outside the command line is missing -- the device, or
    (with one) the map file named here, which does not exist.  Exit status 2 is the example's own refusal of its arguments."""
    r = subprocess.run([EXE, *args, "--hdr", str(tmp_path / "no_such_map.hdr"), "--out", str(tmp_path / "frame.png")], text=True, capture_output=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "unknown argument" not in r.stderr and "wants" not in r.stderr and "not with" not in r.stderr, r.stderr
    assert not (tmp_path / "frame.png").exists()


def write_hdr(path, img):
    """flat (uncompressed) Radiance RGBE, rows top-down in the file (-Y); img rows are bottom-up like trc_host_load_hdr's result"""
    top_down = img[::-1]
    m = top_down.max(axis=2)
    mant, expo = np.frexp(m)
    ok = m > 1e-32
    scale = np.where(ok, mant * 256.0 / np.where(ok, m, 1), 0)
    rgbe = np.zeros(top_down.shape[:2] + (4,), np.uint8)
    rgbe[..., :3] = np.clip(top_down * scale[..., None], 0, 255).astype(np.uint8)
    rgbe[..., 3] = np.where(ok, expo + 128, 0).astype(np.uint8)
    h, w = img.shape[:2]
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode() + rgbe.tobytes())


@pytest.mark.gpu
def test_example_renders_an_env_lit_panorama_and_denoises_along_the_rays(tmp_path):
    from PIL import Image
    W, H = 104, 72
    ys, xs = np.mgrid[0:16, 0:32]
    sky = np.stack([0.2 + 0.02 * ys, 0.3 + 0.01 * xs, 0.5 + 0.0 * xs], axis=-1).astype(np.float32)      # no black texel
    sky[12, 20] = (300.0, 280.0, 200.0)                                                                  # a sun
    write_hdr(str(tmp_path / "sky.hdr"), sky)
    out = tmp_path / "frame.png"
    r = subprocess.run([EXE, "--scene", "spheres", "--size", str(W), str(H), "--spp", "16", "--integrator", "mis", "--hdr", str(tmp_path / "sky.hdr"), "--env-light",
                        "--projection", "equirect", "--aa", "2", "--denoise", "--out", str(out)], text=True, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert re.search(r"camera rays: 2 sets, equirectangular, ", r.stdout) and "denoiser guided by the camera rays" in r.stdout, r.stdout
    assert re.search(r"mean history length 1\.00 over (\d+) hit pixels", r.stdout), r.stdout
    frame = np.asarray(Image.open(str(out)).convert("RGBA"))
    assert frame.shape == (H, W, 4) and frame[..., :3].any()
