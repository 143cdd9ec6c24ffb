"""The definition of trc_recompute_normals (include/tracer_abi.h) restated in numpy, operation by operation, float32 throughout, for
tests/test_normals_cpu.py and tests/test_gpu_recompute_normals.py: the corner list of every vertex from the index array (ascending),
the face terms cross(p1 - p0, p2 - p0), their sum in corner order from +0, the side of the normal the vertex holds, the division by
the correctly rounded length, the vertices that keep their bits, and the restriction to a range.  The steps are functions of their
own, so that a near miss replaces one of them and keeps the rest."""
import numpy as np

F = np.float32


def adjacency(indices, n_vertex):
    """(offsets, corners): corners[offsets[v]:offsets[v + 1]] are the k with indices[k] == v, ascending in k"""
    idx = np.asarray(indices, dtype=np.uint32).ravel()
    corners = np.argsort(idx, kind="stable").astype(np.uint32)
    offsets = np.searchsorted(idx[corners], np.arange(n_vertex + 1), side="left").astype(np.uint32)
    return offsets, corners


def valences(indices, n_vertex):
    offsets, _ = adjacency(indices, n_vertex)
    return (offsets[1:] - offsets[:-1]).astype(np.int64)


def edges(vertices, indices):
    """(e1, e2) per triangle: p1 - p0 and p2 - p0 in index-list order"""
    p = np.ascontiguousarray(vertices, dtype=F)[:, :3]
    tri = np.asarray(indices, dtype=np.uint32).reshape(-1, 3)
    return p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]]


def face_terms(vertices, indices):
    """c = cross(e1, e2) per triangle: two products and one difference per component, each rounded"""
    e1, e2 = edges(vertices, indices)
    c = np.empty_like(e1)
    c[:, 0] = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    c[:, 1] = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    c[:, 2] = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return c


def vertex_sums(c, indices, n_vertex, descending=False, dtype=F):
    """s[v] = ((+0 + c(k0 / 3)) + c(k1 / 3)) + ... over v's corners in ascending (or descending) order.  Step j adds the j-th corner of
    every vertex that has one: the order WITHIN a vertex is the list's"""
    offsets, corners = adjacency(indices, n_vertex)
    val = (offsets[1:] - offsets[:-1]).astype(np.int64)
    s = np.zeros((n_vertex, 3), dtype)
    c = c.astype(dtype)
    for j in range(int(val.max()) if n_vertex else 0):
        m = np.nonzero(val > j)[0]
        k = offsets[m] + (val[m] - 1 - j if descending else j)
        s[m] = s[m] + c[corners[k] // 3]
    return s


def side(s, n_cur, enabled=True):
    """-s where d = (s.x n.x + s.y n.y) + s.z n.z < 0, s elsewhere (d == 0 and NaN included) -> (s, flipped)"""
    with np.errstate(all="ignore"):
        d = (s[:, 0] * n_cur[:, 0] + s[:, 1] * n_cur[:, 1]) + s[:, 2] * n_cur[:, 2]
    flipped = (d < 0) & enabled
    return np.where(flipped[:, None], -s, s), flipped


def by_division(s):
    """(n, ok): n = s / l with l = sqrt((s.x s.x + s.y s.y) + s.z s.z); ok where l is finite and > 0"""
    with np.errstate(all="ignore"):
        q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        l = np.sqrt(q)
        ok = np.isfinite(l) & (l > 0)
        return s / l[:, None], ok


def in_range(n_vertex, first, count):
    m = np.zeros(n_vertex, bool)
    m[first:first + count] = True
    return m


def recompute(vertices, indices, first=0, count=None, terms=face_terms, sums=vertex_sums, side_rule=True, normalise=by_division):
    """(n, 8) float32 vertices with the normals of [first, first + count) re-derived; everything else keeps its bits.  The keyword
    arguments replace a step of the definition (the near misses of tests/test_normals_cpu.py)"""
    v = np.ascontiguousarray(vertices, dtype=F).copy()
    n = len(v)
    count = n - first if count is None else count
    assert valid_range(first, count, n)
    s = sums(terms(v, indices), indices, n)
    assert s.dtype == F
    s, _ = side(s, v[:, 3:6], side_rule)
    new, ok = normalise(s)
    m = ok & in_range(n, first, count)
    v[m, 3:6] = new[m].astype(F)
    return v


def kept(vertices, indices):
    """the vertices that keep their bits whatever the range: no corner, no area, a length that is not finite or not > 0"""
    v = np.ascontiguousarray(vertices, dtype=F)
    s = vertex_sums(face_terms(v, indices), indices, len(v))
    return np.nonzero(~by_division(s)[1])[0]


def flipped(vertices, indices):
    """the vertices whose sum the side rule negates"""
    v = np.ascontiguousarray(vertices, dtype=F)
    return np.nonzero(side(vertex_sums(face_terms(v, indices), indices, len(v)), v[:, 3:6])[1])[0]


def valid_range(first, count, n_vertex):
    """what tracer_amd/csrc/normals_check.hpp accepts: an empty range anywhere, else one that ends within n_vertex"""
    return count == 0 or (0 <= first <= n_vertex and 0 <= count <= n_vertex - first)


def key_bits(n_vertex):
    """the key bits the adjacency build's sort looks at (normals_check.hpp)"""
    return max(1, int(max(n_vertex - 1, 0)).bit_length())


HUB_VALENCE = 70


def fan():
    """(vertices, indices, planted): a fan for host.Mesh.from_arrays -- a hub of valence 70 (past a wavefront's width and any unroll
    factor) over a rim that is neither flat nor round, so that no two triangles share area or plane.  planted: 'hub'; 'unnamed', a
    vertex no triangle names; 'zero_area', two vertices at one position that a single triangle of no area names; 'twice', a rim vertex
    that one triangle names twice; 'opposed', the rim vertices both of whose fan triangles are wound against the stored normals IN THE
    SCENE -- HostScene mirrors z, which turns every winding round, so here they are the ones wound WITH them.  The rim's radius is twice
    as large on the other half, so that the hub and the two rim vertices between the halves follow the larger triangles"""
    n_rim = HUB_VALENCE
    theta = 2.0 * np.pi * np.arange(n_rim) / n_rim
    radius = np.where(np.arange(n_rim) <= n_rim // 2, 0.12, 0.06) * (1.0 + 0.1 * np.sin(5.0 * theta + 1.0))
    v = np.zeros((n_rim + 4, 8), np.float64)
    v[0, :6] = (0.0, 0.03, 0.0, 0.0, 1.0, 0.0)
    # (the height changes slowly along the rim: refit_ref.twist turns a vertex by its height, and neighbours must not overtake each other)
    v[1:n_rim + 1, 0] = radius * np.cos(theta); v[1:n_rim + 1, 1] = 0.02 * np.sin(theta + 0.5); v[1:n_rim + 1, 2] = radius * np.sin(theta)
    v[1:n_rim + 1, 3] = 0.1 * np.cos(theta); v[1:n_rim + 1, 4] = 1.0; v[1:n_rim + 1, 5] = 0.1 * np.sin(theta)
    unnamed, z0, z1 = n_rim + 1, n_rim + 2, n_rim + 3
    v[unnamed, :6] = (0.01, 0.0, 0.01, 0.0, 1.0, 0.0)
    v[z0, :6] = v[z1, :6] = (0.02, 0.01, -0.02, 0.6, 0.8, 0.0)
    v[:, 6] = 0.5 + 2.0 * v[:, 0]; v[:, 7] = 0.5 + 2.0 * v[:, 2]
    tris = []
    for j in range(n_rim):
        a, b = 1 + j, 1 + (j + 1) % n_rim
        tris.append((0, a, b) if j < n_rim // 2 else (0, b, a))      # (0, a, b): cross points to -y here, to +y in the scene
    twice = 1 + 10
    tris.append((z0, z1, 1 + 3))                                     # no area: two of its vertices are one point
    tris.append((twice, twice, 1 + 11))                              # ... and here two of its corners are one vertex
    planted = {"hub": 0, "unnamed": unnamed, "zero_area": (z0, z1), "twice": twice,
               "opposed": tuple(1 + j for j in range(n_rim // 2 + 1, n_rim))}
    return v.astype(F), np.asarray(tris, np.uint32).ravel(), planted
