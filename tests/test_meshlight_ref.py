"""CPU restatement of TRC_FLAG_MESH_LIGHTS (tests/meshlight_ref): the alias table reproduces weight / total to the granularity of its
32-bit thresholds, pdfA * A sums to 1 over the lights, sampled points lie in their triangle, triangles that are no lights (degenerate,
NaN vertex, zero albedo, another material type) are left out, and the picked triangles follow the weights (chi-square).  No GPU:
tests/test_gpu_mesh_lights.py holds the kernels to this restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "meshlight_ref"))
import meshlight_loader as ml  # noqa: E402

F = np.float32
MAT_DIFFUSE, MAT_LAMBERT = 0, 1


@pytest.fixture(scope="module")
def ref():
    return ml.build()


def random_mesh(rng, n, n_mat=6):
    """n random triangles of very different sizes; materials 0 .. n_mat - 1: even ones emitters of random radiance, odd ones Lambert"""
    centre = rng.uniform(-5, 5, size=(n, 1, 3))
    size = np.exp(rng.uniform(-4, 1, size=(n, 1, 1)))
    tri_v = (centre + size * rng.normal(size=(n, 3, 3))).astype(F)
    mat_type = np.array([MAT_DIFFUSE if k % 2 == 0 else MAT_LAMBERT for k in range(n_mat)], np.int32)
    mat_albedo = (rng.random((n_mat, 3)) * 10).astype(F)
    tri_mat = rng.integers(0, n_mat, size=n).astype(np.uint32)
    return tri_v, tri_mat, mat_type, mat_albedo


def lum(albedo):
    a = np.asarray(albedo, np.float64)
    return 0.212671 * a[..., 0] + 0.715160 * a[..., 1] + 0.072169 * a[..., 2]


@pytest.mark.parametrize("n", [1, 2, 7, 500, 20000])
def test_alias_table_reproduces_weights(ref, n):
    rng = np.random.default_rng(n)
    tri_v, tri_mat, mat_type, mat_albedo = random_mesh(rng, n)
    if n == 1:
        tri_mat[:] = 0
    t = ref.tables(tri_v, tri_mat, mat_type, mat_albedo)
    lights = np.flatnonzero(mat_type[tri_mat] == MAT_DIFFUSE)
    assert t["n_lights"] == len(lights) and np.array_equal(t["tri"], lights)          # in triangle order
    if len(lights) == 0:
        assert t["total"] == 0 and not t["pdfA"].any()
        return
    A = ml.tri_areas(tri_v)[lights]
    w = lum(mat_albedo[tri_mat[lights]]) * A
    assert np.isclose(t["total"], w.sum(), rtol=1e-5)
    p = ml.alias_probabilities(t["alias"])
    nl = len(lights)
    # each entry's keep and alias shares are quantised to 2^-32 / n; the float32 inputs (y, A) carry ~1e-6 relative error
    assert np.abs(p - w / w.sum()).max() < 4 * 2.0 ** -32 + 3e-6 * (w / w.sum()).max()
    assert t["alias"][:, 1].max() < nl
    # pdfA * A sums to 1 over the lights, within the rounding of n float32 terms
    pdfA = t["pdfA"].astype(np.float64)
    assert np.all(pdfA[np.setdiff1d(np.arange(n), lights)] == 0) and np.all(pdfA[lights] > 0)
    assert abs((pdfA[lights] * A).sum() - 1.0) < 2e-6 * np.sqrt(nl) + 1e-6
    assert np.allclose(pdfA[lights], lum(mat_albedo[tri_mat[lights]]) / w.sum(), rtol=1e-5)


def test_no_lights_excluded_triangles(ref):
    """degenerate, NaN-vertex, infinite, zero-albedo, negative-albedo, non-emitter and out-of-table triangles are no lights"""
    good = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    tri_v = np.stack([good, np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], F),            # collinear: area 0
                      np.array([[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]], F), good, good, good, good,
                      np.array([[0, 0, 0], [3e38, 0, 0], [0, 3e38, 0]], F), good * 2])
    mat_type = np.array([MAT_DIFFUSE, MAT_DIFFUSE, MAT_LAMBERT, MAT_DIFFUSE, MAT_DIFFUSE], np.int32)
    mat_albedo = np.array([[1, 1, 1], [0, 0, 0], [5, 5, 5], [-1, -1, -1], [np.inf, 1, 1]], F)
    tri_mat = np.array([0, 0, 0, 1, 2, 3, 4, 0, 0], np.uint32)
    t = ref.tables(tri_v, tri_mat, mat_type, mat_albedo)
    assert t["n_lights"] == 2 and list(t["tri"]) == [0, 8]
    assert np.all(t["pdfA"][1:8] == 0) and np.all(np.isfinite(t["pdfA"]))
    assert np.isclose(t["total"], 0.5 + 2.0, rtol=1e-6)                               # y = 1 (the three coefficients sum to 1), areas 1/2 and 2
    tri_mat[:] = 9                                                                     # beyond the table
    assert ref.tables(tri_v, tri_mat, mat_type, mat_albedo)["n_lights"] == 0
    t0 = ref.tables(np.zeros((0, 3, 3), F), np.zeros(0, np.uint32), mat_type, mat_albedo)
    assert t0["n_lights"] == 0 and t0["total"] == 0


def test_sampled_points_lie_in_their_triangle(ref):
    rng = np.random.default_rng(3)
    tri_v, tri_mat, mat_type, mat_albedo = random_mesh(rng, 300)
    t = ref.tables(tri_v, tri_mat, mat_type, mat_albedo)
    d = ml.edge_draws(rng, 200000)
    pos = rng.uniform(-8, 8, size=(d.shape[0], 3)).astype(F)
    tri, out = ref.sample(t, d, pos)
    assert np.all(np.isin(tri, t["tri"]))
    v = tri_v[tri].astype(np.float64)
    p, n = out[:, :3].astype(np.float64), out[:, 3:6].astype(np.float64)
    # barycentrics of p by least squares in the triangle's plane
    e1, e2, r = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], p - v[:, 0]
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (r * e1).sum(1), (r * e2).sum(1)
    det = d11 * d22 - d12 * d12
    b1, b2 = (d22 * r1 - d12 * r2) / det, (d11 * r2 - d12 * r1) / det
    scale = np.abs(v).max(axis=(1, 2))
    tol = 1e-5
    assert b1.min() > -tol and b2.min() > -tol and (b1 + b2).max() < 1 + tol
    g = np.cross(e1, e2)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert np.abs((r * g).sum(1)).max() < 1e-5 * scale.max()                           # in the plane
    assert np.allclose(np.abs((n * g).sum(1)), 1.0, atol=1e-5)                        # the unit geometric normal ...
    side = ((pos.astype(np.float64) - p) * n).sum(1)
    assert np.all(side >= -1e-4 * np.linalg.norm(pos.astype(np.float64) - p, axis=1))  # ... turned to the shading point
    assert np.array_equal(out[:, 6], t["pdfA"][tri])
    # the stated barycentrics themselves are in [0, 1] for every draw, the edge values included
    f0, f1 = d[:, 2].view(F), d[:, 3].view(F)
    s = np.sqrt(f0, dtype=F)
    b0_, b1_ = F(1) - s, f1 * s
    b2_ = (F(1) - b0_) - b1_
    for b in (b0_, b1_, b2_):
        assert b.min() >= 0 and b.max() <= 1


def test_picked_triangles_follow_the_weights(ref):
    rng = np.random.default_rng(8)
    tri_v, tri_mat, mat_type, mat_albedo = random_mesh(rng, 400)
    t = ref.tables(tri_v, tri_mat, mat_type, mat_albedo)
    n = 4 * 10 ** 6
    d = np.zeros((n, 4), np.uint32)
    d[:, :2] = rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    d[:, 2:] = np.full((n, 2), 0.25, F).view(np.uint32)
    tri, _ = ref.sample(t, d, np.zeros((n, 3), F))
    A = ml.tri_areas(tri_v)
    w = np.zeros(len(tri_v))
    w[t["tri"]] = lum(mat_albedo[tri_mat[t["tri"]]]) * A[t["tri"]]
    hist = np.bincount(tri, minlength=len(tri_v)).astype(np.float64)
    assert hist[w == 0].sum() == 0
    e = w / w.sum() * n
    keep = e > 5
    chi2 = ((hist[keep] - e[keep]) ** 2 / e[keep]).sum()
    dof = keep.sum() - 1
    # chi-square: mean dof, sd sqrt(2 dof); 6 sd
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)
