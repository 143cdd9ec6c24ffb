"""The definition of trc_morph_vertices (include/tracer_abi.h) restated in numpy, for tests/test_morph_cpu.py and
tests/test_gpu_morph_vertices.py.  Everything is a float32 array and every line is ONE operation, so nothing is fused and the order is
the header's: the active list is the targets k, ascending, whose weight is not zero; for each of them  p = w_k * d[k];  acc = acc + p
on the six values x y z nx ny nz, starting from the rest values.  A vertex under no active target is the rest vertex bit for bit.

Deltas are (n_targets, count, 6) float32: deltas[k, i] belongs to vertex first + i.  Vertices are (n, 8) float32 rows: position,
normal, uv.  The composition with a skin is skin_ref's expressions on the morphed values in place of the rest values."""
import numpy as np

import skin_ref as sr

F = np.float32
MAX_TARGETS = 1024


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def active(weights):
    """[(k, w_k)] for the weights that are not zero (neither +0 nor -0 counts), k ascending"""
    w = _f(weights).ravel()
    return [(int(k), w[k]) for k in range(len(w)) if w[k] != 0]


def morphed_values(rest, first, deltas, weights):
    """-> (n, 8): `rest` with rows [first, first + count) morphed"""
    out = _f(rest).copy()
    deltas = _f(deltas)
    count = deltas.shape[1]
    acc = out[first:first + count, :6].copy()
    for k, w in active(weights):
        p = w * deltas[k]
        acc = acc + p
        assert p.dtype == F and acc.dtype == F
    out[first:first + count, :6] = acc
    return out


def morph(rest, current, first, deltas, weights):
    """rest, current: (n, 8) float32; -> the vertices after trc_morph_vertices(weights, n_bones = 0) under the binding (first, deltas):
    the bound range from REST, the others as in current"""
    out = _f(current).copy()
    count = _f(deltas).shape[1]
    out[first:first + count] = morphed_values(rest, first, deltas, weights)[first:first + count]
    return out


def morph_skin(rest, current, first, deltas, weights, skin_first, bones_idx, skin_weights, palette):
    """-> the vertices after trc_morph_vertices(weights, palette): a vertex of the morph binding is morphed, a vertex of the skin binding
    (skin_first, bones_idx, skin_weights) then gets skin_ref's expressions on what it has by then -- its morphed values or its rest
    values -- and a vertex in neither binding stays as in current"""
    staged = morphed_values(rest, first, deltas, weights)              # rest outside the morph binding
    out = morph(rest, current, first, deltas, weights)
    return sr.skin(staged, out, skin_first, bones_idx, skin_weights, palette)


def valid_binding(first, deltas, n_vertex):
    """what trc_morph_bind accepts (TRC_OK) on a scene with n_vertex > 0 vertices; a refusal is TRC_ERR_INVALID_ARG.  An empty table
    removes the binding, whatever `first`."""
    d = _f(deltas)
    if d.shape[0] == 0 or d.shape[1] == 0:
        return True
    if first + d.shape[1] > n_vertex or d.shape[0] > MAX_TARGETS:
        return False
    return bool(np.isfinite(d).all())


def valid_weights(weights, n_targets):
    w = _f(weights).ravel()
    return len(w) == n_targets and bool(np.isfinite(w).all())


# ---------------------------------------------------------------------------------------------------- data for the tests
def deltas(n_targets, count, seed=5):
    """(n_targets, count, 6) float32, inexact in float32 and about as large as the rest values they are added to (a few units of the
    Cornell scene's hundreds), so that every sum rounds; every 9th delta of a target has a component of exactly 0"""
    rng = np.random.default_rng(seed)
    d = (rng.random((n_targets, count, 6)) * 6.0 - 3.0).astype(F)
    d[:, :, 3:] *= F(0.11)                                              # the normals' deltas: a tenth of a unit normal
    d[:, 4::9, 1] = F(0)
    return d


WEIGHT_KINDS = ("all", "alternating", "negative", "zero")


def weights(n_targets, kind, seed=7):
    """all: none is zero.  alternating: every odd target has weight +0 or -0 (the compaction).  negative: like all with every other
    weight below zero.  zero: all +0 / -0."""
    rng = np.random.default_rng(seed + n_targets)
    w = (rng.random(n_targets) * 0.9 + 0.07).astype(F)
    k = np.arange(n_targets)
    if kind == "alternating":
        w[k % 2 == 1] = F(0)
        w[k % 4 == 3] = F(-0.0)
    elif kind == "negative":
        w[k % 2 == 0] = -w[k % 2 == 0]
    elif kind == "zero":
        w[:] = F(0)
        w[1::2] = F(-0.0)
    else:
        assert kind == "all"
    return w
