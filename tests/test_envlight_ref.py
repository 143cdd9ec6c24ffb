"""CPU restatement of TRC_FLAG_ENV_LIGHT (tests/envlight_ref): the alias tables reproduce the normalised cell weights (checked
against float64 numpy), the pdf integrates to 1 over the sphere, a sample's pdf is the pdf of its direction, and edge maps
(1x1, 1xN, Nx1, black rows, one hot texel, all black) give sound tables.  No GPU: tests/test_gpu_envlight.py holds the kernels
to this restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envlight_ref"))
import envlight_loader as el  # noqa: E402


@pytest.fixture(scope="module")
def ref():
    return el.build()


def alias_probabilities(tab):
    """probability of every entry of an alias table ({threshold, alias} pairs), exactly as the sampler's integer draws give it"""
    n = tab.shape[0]
    keep = (tab[:, 0].astype(np.float64)) / 2.0 ** 32
    p = keep / n
    np.add.at(p, tab[:, 1].astype(np.int64), (1.0 - keep) / n)
    return p


def numpy_weights(rgb):
    H, W = rgb.shape[:2]
    y = (np.float32(0.212671) * rgb[..., 0] + np.float32(0.715160) * rgb[..., 1]) + np.float32(0.072169) * rgb[..., 2]
    y = np.where((y > 0) & np.isfinite(y), y, 0).astype(np.float64)
    pad = np.pad(y, 1, mode="edge")
    m = np.max([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    lat = np.pi * ((np.arange(H) + 0.5) / H - 0.5)
    return m * np.cos(lat)[:, None]


def maps():
    rng = np.random.default_rng(5)
    out = {
        "random": rng.random((48, 96, 3), dtype=np.float32) * 3,
        "sun_sky": el.sun_sky(128, 64),
        "1x1": np.full((1, 1, 3), 2.0, np.float32),
        "1xN": rng.random((1, 17, 3), dtype=np.float32),
        "Nx1": rng.random((13, 1, 3), dtype=np.float32),
        "black_rows": rng.random((20, 30, 3), dtype=np.float32),
        "hot_texel": np.zeros((32, 64, 3), np.float32),
        "negative_nan": rng.random((16, 16, 3), dtype=np.float32) - 0.3,
    }
    out["black_rows"][3:9] = 0
    out["black_rows"][-1] = 0
    out["hot_texel"][20, 40] = (1e4, 1e4, 1e4)
    out["negative_nan"][2, 3, 1] = np.nan
    out["negative_nan"][7, 7, 0] = np.inf
    return out


@pytest.mark.parametrize("name", list(maps()))
def test_tables_reproduce_weights(ref, name):
    rgb = maps()[name]
    t = ref.tables(rgb)
    H, W = rgb.shape[:2]
    w64 = numpy_weights(rgb)
    assert np.allclose(t["weight"], w64, rtol=2e-5, atol=0)       # float32 cos of the cell centre's latitude
    assert t["total"] > 0
    assert np.isclose(t["total"], t["weight"].astype(np.float64).sum(), rtol=1e-12)
    # marginal over rows x conditional in the row = the normalised weights, to the 2^-32 resolution of the decisions
    pm = alias_probabilities(t["marg"])
    cell = np.stack([alias_probabilities(t["rows"][j]) for j in range(H)]) * pm[:, None]
    target = t["weight"].astype(np.float64) / t["weight"].astype(np.float64).sum()
    assert np.abs(cell - target).max() < 4 * (W + H) * 2.0 ** -32 + 1e-12
    assert t["rows"][..., 1].max() < W and t["marg"][:, 1].max() < H
    # zero-weight cells get (almost) nothing
    assert np.all(cell[target == 0] <= (W + H) * 2.0 ** -32)


def test_all_black_map(ref):
    t = ref.tables(np.zeros((8, 16, 3), np.float32))
    assert t["total"] == 0 and not t["weight"].any()
    draws = np.random.default_rng(0).integers(0, 2 ** 32, size=(100, 6), dtype=np.uint64).astype(np.uint32)
    draws[:, 4:] = np.float32(0.5).view(np.uint32)
    assert not ref.sample(t, draws)[:, 3].any()
    assert not ref.pdf(t, np.array([[0, 1, 0], [1, 0, 0]], np.float32)).any()


def random_draws(rng, n):
    d = rng.integers(0, 2 ** 32, size=(n, 6), dtype=np.uint64).astype(np.uint32)
    d[:, 4:] = (rng.integers(0, 2 ** 24, size=(n, 2)).astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)
    return d


@pytest.mark.parametrize("name", ["random", "sun_sky", "hot_texel", "black_rows", "1xN", "Nx1"])
def test_pdf_integrates_to_one(ref, name):
    t = ref.tables(maps()[name])
    # midpoint rule on a fine (phi, latitude) grid: d(omega) = cos(lat) dphi dlat
    n_phi, n_lat = 1024, 512
    phi = 2 * np.pi * ((np.arange(n_phi) + 0.5) / n_phi - 0.5)
    lat = np.pi * ((np.arange(n_lat) + 0.5) / n_lat - 0.5)
    P, L = np.meshgrid(phi, lat)
    d = np.stack([np.cos(L) * np.cos(P), np.sin(L), np.cos(L) * np.sin(P)], -1).reshape(-1, 3).astype(np.float32)
    pdf = ref.pdf(t, d).astype(np.float64).reshape(n_lat, n_phi)
    integral = (pdf * np.cos(L)).sum() * (2 * np.pi / n_phi) * (np.pi / n_lat)
    assert abs(integral - 1.0) < 2e-3, integral


@pytest.mark.parametrize("name", ["random", "sun_sky", "hot_texel", "black_rows"])
def test_sample_pdf_round_trip(ref, name):
    t = ref.tables(maps()[name])
    H, W = t["weight"].shape
    out = ref.sample(t, random_draws(np.random.default_rng(3), 200000))
    d, p = out[:, :3], out[:, 3]
    assert np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6)
    assert np.all(p > 0)                                       # a sample never lands on a zero-weight cell
    # away from cell edges the pdf function gives the sample's pdf
    u = np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi) + 0.5
    w = np.arcsin(np.clip(d[:, 1], -1, 1)) / np.pi + 0.5
    inner = (np.abs(u * W - np.round(u * W)) > 1e-3) & (np.abs(w * H - np.round(w * H)) > 1e-3) & (np.abs(d[:, 1]) < 0.999)
    assert inner.mean() > 0.9
    q = ref.pdf(t, d[inner])
    assert np.allclose(q, p[inner], rtol=1e-4)


def test_hot_texel_samples_stay_near_it(ref):
    t = ref.tables(maps()["hot_texel"])
    out = ref.sample(t, random_draws(np.random.default_rng(4), 10000))
    H, W = t["weight"].shape
    u = np.arctan2(out[:, 2], out[:, 0]) / (2 * np.pi) + 0.5
    w = np.arcsin(np.clip(out[:, 1], -1, 1)) / np.pi + 0.5
    assert np.all(np.abs(u * W - 40.5) <= 1.5 + 1e-3) and np.all(np.abs(w * H - 20.5) <= 1.5 + 1e-3)
