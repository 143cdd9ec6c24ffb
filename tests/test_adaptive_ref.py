"""The restatement of the per-tile error estimate (tests/adaptive_ref.py) against tiles computed by hand, its independence of the order
of the pixels, the ctypes mirror of the new structs against the header, and the new symbols in the shared libraries.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import adaptive_ref as ar
from conftest import ROOT
from tracer_amd import abi, device

F = np.float32
NEW = ["trc_set_tile_mask", "trc_download_tile_mask", "trc_tile_snapshot", "trc_tile_error", "trc_download_tile_error",
       "trc_adaptive_default_params", "trc_render_adaptive", "trc_download_tile_samples"]


def planes(W, H, value):
    p = np.zeros((H, W, 4), dtype=F)
    p[..., :3] = value
    return p


def test_a_tile_that_did_not_move_has_no_error():
    I = planes(16, 16, (0.25, 0.5, 0.125))
    assert ar.tile_errors(I, I.copy()).tolist() == [0.0]


def test_a_uniform_tile_by_hand():
    # d = 3 * 0.125 = 0.375, s = 3 * 0.75 = 2.25, sqrt = 1.5, e = 0.25: every step exact in binary32
    I, A = planes(16, 16, 0.75), planes(16, 16, 0.625)
    assert ar.pixel_q(I, A)[0, 0] == 0.25 * 65536
    assert ar.tile_errors(I, A).tolist() == [0.25]
    # ... and a pixel whose quotient is not a multiple of 2^-16 is truncated, not rounded: d = 1, s' = 9 -> e = fl(1 / 3)
    I, A = planes(1, 1, (5.0, 3.0, 1.0)), planes(1, 1, (4.0, 3.0, 1.0))
    e = F(1.0) / F(3.0)
    assert ar.pixel_q(I, A)[0, 0] == int(math.floor(float(e) * 65536.0)) == 21845
    assert ar.tile_errors(I, A)[0] == F(21845 / 65536.0)


def test_a_dark_pixel_divides_by_the_root_of_the_eps():
    # s = 3e-5 < 1e-4: e = d / sqrt(fl(1e-4)), in binary32
    I, A = planes(16, 16, 1e-5), planes(16, 16, 0.0)
    v = F(1e-5)
    d = (v + v) + v
    e = d / np.sqrt(F(1e-4))
    assert ar.pixel_q(I, A)[3, 5] == int(float(e * F(65536.0)))
    assert ar.tile_errors(I, A)[0] == F(np.float64(256 * int(float(e * F(65536.0)))) / (256.0 * 65536.0))
    # a negative sum takes the eps too, and |I - A| is taken per channel
    I, A = planes(1, 1, (-2.0, 0.5, 0.5)), planes(1, 1, (0.0, 0.0, 0.0))
    e = F(3.0) / np.sqrt(F(1e-4))
    assert ar.pixel_q(I, A)[0, 0] == int(float(e * F(65536.0)))


def test_nan_and_inf_pixels_take_the_cap():
    A = planes(16, 16, 0.5)
    I = A.copy()
    I[2, 3, 0] = np.nan          # d and s NaN: s takes the eps, e is NaN -> the cap
    I[4, 5, 1] = np.inf          # d = inf, s = inf: inf / inf = NaN -> the cap
    I[6, 7, 2] = -np.inf         # d = inf, s = -inf -> eps: e = inf -> the cap
    A[8, 9, 0] = np.nan          # d NaN with a finite s
    q = ar.pixel_q(I, A)
    cap = 65535 * 65536
    assert [int(q[2, 3]), int(q[4, 5]), int(q[6, 7]), int(q[8, 9])] == [cap] * 4
    assert int(q.sum()) == 4 * cap                          # every other pixel did not move
    assert ar.tile_errors(I, A)[0] == F(np.float64(4 * cap) / (256.0 * 65536.0))
    assert np.isfinite(ar.tile_errors(I, A)).all()


def test_a_partial_tile_divides_by_its_own_pixel_count():
    # 40 x 36: 3 x 3 tiles, the last column 8 wide, the last row 4 high
    W, H = 40, 36
    assert ar.tile_grid(W, H) == (3, 3)
    assert ar.tile_pixels(W, H).tolist() == [256, 256, 128, 256, 256, 128, 64, 64, 32]
    I, A = planes(W, H, 0.75), planes(W, H, 0.625)
    assert ar.tile_errors(I, A).tolist() == [0.25] * 9      # a mean, whatever N_t is
    I[35, 39, :3] = 0.625                                   # one pixel of the 8 x 4 corner tile did not move
    E = ar.tile_errors(I, A)
    assert E[8] == F(31 * 0.25 / 32) and E[:8].tolist() == [0.25] * 8
    # tiles outside the mask keep what they had
    mask = np.zeros(9, dtype=np.uint8); mask[8] = 1
    prev = np.arange(9, dtype=F)
    got = ar.tile_errors(I, A, mask, prev)
    assert got[:8].tolist() == prev[:8].tolist() and got[8] == E[8]


def test_permuting_the_pixels_of_a_tile_changes_no_bit():
    rs = np.random.RandomState(5)
    I = rs.gamma(0.3, 2.0, size=(16, 16, 4)).astype(F)
    A = (I * rs.uniform(0.5, 1.5, size=I.shape)).astype(F)
    I[1, 1, 0] = np.nan; I[2, 2, 1] = np.inf; I[3, 3, :3] = 0.0
    want = ar.tile_errors(I, A)[0]
    for seed in range(8):
        perm = np.random.RandomState(seed).permutation(256)
        Ip, Ap = I.reshape(256, 4)[perm].reshape(16, 16, 4), A.reshape(256, 4)[perm].reshape(16, 16, 4)
        assert ar.tile_errors(Ip, Ap)[0].view(np.uint32) == want.view(np.uint32)


def test_the_loop_over_renders_that_never_move_stops_every_tile_at_the_first_check():
    frame = (planes(40, 36, 0.5), np.zeros((36, 40, 4), np.uint32))
    r = ar.adaptive_loop(lambda n: frame, 40, 36, 8, 64, 0.01)
    assert r["passes"] == 2 and r["active_tiles"] == 0 and r["n_t"].tolist() == [16] * 9 and r["samples"] == 40 * 36 * 16
    # ... and renders that keep moving run to max_spp, which need not be h0 * 2^k
    seen = []
    def moving(n):
        seen.append(n)
        return planes(40, 36, float(n)), np.full((36, 40, 4), n, np.uint32)
    r = ar.adaptive_loop(moving, 40, 36, 8, 40, 0.01)
    assert seen == [8, 16, 32, 40] and r["passes"] == 4 and r["active_tiles"] == 9 and r["n_t"].tolist() == [40] * 9
    assert (r["rng"] == 40).all() and r["max_error"] == r["E"].max() > 0


def test_ctypes_structs_have_the_header_s_sizes_and_offsets(tmp_path):
    off = lambda t, f: getattr(t, f).offset
    assert C.sizeof(abi.AdaptiveParams) == 16 and off(abi.AdaptiveParams, "max_spp") == 4 and off(abi.AdaptiveParams, "reserved") == 8
    assert C.sizeof(abi.AdaptiveReport) == 24 and off(abi.AdaptiveReport, "active_tiles") == 4 and off(abi.AdaptiveReport, "samples") == 8
    assert off(abi.AdaptiveReport, "max_error") == 16
    # ... which the header states itself: a C program prints them
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "tracer_abi.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %g %d\\n", sizeof(trc_adaptive_params),'
                   ' offsetof(trc_adaptive_params, max_spp), offsetof(trc_adaptive_params, reserved), sizeof(trc_adaptive_report),'
                   ' offsetof(trc_adaptive_report, active_tiles), offsetof(trc_adaptive_report, samples), offsetof(trc_adaptive_report, max_error),'
                   ' (double)TRC_ADAPTIVE_EPS, TRC_TILE);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert [int(v) for v in out[:7]] == [16, 4, 8, 24, 4, 8, 16]
    assert F(float(out[7])) == ar.EPS == F(abi.ADAPTIVE_EPS) and int(out[8]) == ar.TILE == abi.TRC_TILE


def test_default_params_come_from_the_header():
    a = abi.AdaptiveParams()
    device.lib().trc_adaptive_default_params(C.byref(a))
    text = open(os.path.join(ROOT, "include", "tracer_abi.h")).read()
    stated = re.search(r"#define TRC_ADAPTIVE_DEFAULT_THRESHOLD ([0-9.e-]+)f", text).group(1)
    assert a.max_spp == 256 and a.threshold == F(float(stated)) and a.threshold > 0 and list(a.reserved) == [0, 0]


def test_the_four_shared_libraries_export_the_new_symbols():
    for name in NEW:
        assert name in abi.DEVICE_SYMBOLS, name
    exported = lambda path: {line.split()[-1] for line in subprocess.check_output(["nm", "-D", "--defined-only", path], text=True).splitlines() if line.strip()}
    for path in (device.lib_path(), device.fast_lib_path(), device.hooks_lib_path()):
        assert not [s for s in NEW if s not in exported(path)], path
    # the fourth, the host library, gains nothing: the feature is the device's
    from tracer_amd import host
    assert not [s for s in exported(host.lib_path()) if s in NEW]
    for L in (device.lib(), device.lib(fast_math=True), device.lib(hooks=True)):
        for name in NEW:
            getattr(L, name)


def test_knob_is_named_in_the_table_and_in_the_header():
    assert '"mask_forgets_costs"' in open(os.path.join(ROOT, "tracer_amd", "csrc", "trc_abi.hip")).read()
    assert '"mask_forgets_costs"' in open(os.path.join(ROOT, "include", "tracer_abi.h")).read()
