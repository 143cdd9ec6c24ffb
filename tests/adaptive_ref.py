"""The per-tile error estimate and the adaptive driver's loop of include/tracer_abi.h ("Tile mask, per-tile error estimate, adaptive
sampling"), restated in numpy: every step in binary32 in the header's order, the tile sums as integers.  tile_errors is the definition
of trc_tile_error; adaptive_loop is trc_render_adaptive over PLAIN renders: `render(n)` is the frame of a plain n-sample trc_render, and
a tile that stopped at n_t samples holds the pixels of render(n_t)."""
import numpy as np

F = np.float32
TILE = 16
EPS = F(1e-4)                 # TRC_ADAPTIVE_EPS
CAP = F(65535.0)


def tile_grid(W, H):
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def tile_slices(W, H):
    """(t, rows, columns) of every tile, row-major"""
    th, tw = tile_grid(W, H)
    for ty in range(th):
        for tx in range(tw):
            yield ty * tw + tx, slice(ty * TILE, min(H, (ty + 1) * TILE)), slice(tx * TILE, min(W, (tx + 1) * TILE))


def tile_pixels(W, H):
    """N_t of every tile"""
    return np.array([(r.stop - r.start) * (c.stop - c.start) for _, r, c in tile_slices(W, H)], dtype=np.int64)


def pixel_q(I, A):
    """q of every pixel: (..., >= 3) float32 planes I and A -> uint64"""
    I, A = np.asarray(I, dtype=F), np.asarray(A, dtype=F)
    with np.errstate(all="ignore"):
        d = (np.abs(I[..., 0] - A[..., 0]) + np.abs(I[..., 1] - A[..., 1])) + np.abs(I[..., 2] - A[..., 2])
        s = (I[..., 0] + I[..., 1]) + I[..., 2]
        s1 = np.where(s > EPS, s, EPS)              # a NaN s takes the eps
        e = d / np.sqrt(s1)
        e1 = np.where(e < CAP, e, CAP)              # NaN and inf take the cap
        scaled = e1 * F(65536.0)
    assert d.dtype == F and s1.dtype == F and e.dtype == F and scaled.dtype == F
    return scaled.astype(np.uint64)                 # truncation; scaled < 2^32


def tile_value(q):
    """E_t of one tile from the q of its pixels (any shape)"""
    q = np.asarray(q, dtype=np.uint64)
    total = int(q.sum(dtype=np.uint64))
    return F(np.float64(total) / (np.float64(q.size) * 65536.0))


def tile_errors(I, A, mask=None, prev=None):
    """E_t of every tile of `mask` (None: all) of (H, W, >= 3) planes; the other tiles keep prev's value (None: 0) -> (n tiles,) float32"""
    H, W = I.shape[:2]
    th, tw = tile_grid(W, H)
    out = np.zeros(th * tw, dtype=F) if prev is None else np.array(prev, dtype=F).ravel().copy()
    m = np.ones(th * tw, dtype=bool) if mask is None else np.asarray(mask).ravel() != 0
    q = pixel_q(I, A)
    for t, rows, cols in tile_slices(W, H):
        if m[t]:
            out[t] = tile_value(q[rows, cols])
    return out


def adaptive_loop(render, W, H, h0, max_spp, threshold):
    """trc_render_adaptive over plain renders.  render(n) -> (accumulator (H, W, 4) float32, rng (H, W, 4) uint32) of a plain n-sample render.
    -> dict: accum, rng (the composed planes), n_t, E (n tiles,), passes, active_tiles, samples, max_error, first_E (E after the first check)"""
    assert h0 >= 8 and max_spp >= 2 * h0 and threshold > 0
    threshold = F(threshold)
    acc, rng = (a.copy() for a in render(h0))
    A = acc.copy()
    th, tw = tile_grid(W, H)
    mask = np.ones(th * tw, dtype=bool)
    n_t = np.zeros(th * tw, dtype=np.uint32)
    E = np.zeros(th * tw, dtype=F)
    n, passes, first_E = h0, 1, None
    while n < max_spp and mask.any():
        n += min(n, max_spp - n)
        passes += 1
        full_acc, full_rng = render(n)
        for t, rows, cols in tile_slices(W, H):
            if mask[t]:
                acc[rows, cols] = full_acc[rows, cols]; rng[rows, cols] = full_rng[rows, cols]
        E = tile_errors(acc, A, mask, E)
        for t, rows, cols in tile_slices(W, H):
            if mask[t]:
                A[rows, cols] = acc[rows, cols]
        n_t[mask] = n
        mask = mask & ~(E <= threshold)
        if first_E is None:
            first_E = E.copy()
    return dict(accum=acc, rng=rng, snapshot=A, n_t=n_t, E=E, passes=passes, active_tiles=int(mask.sum()),
                samples=int((tile_pixels(W, H) * n_t.astype(np.int64)).sum()), max_error=F(E.max()), first_E=first_E, mask=mask)
