"""tests/sample11_cases.py held to its own conditions, without a GPU: the inputs of tests/test_gpu_sample11_once.py must fall where that
test needs them -- on both sides of sample11's split, into the Newton loop's two exits at small bounds, and onto the special operands
of the corner's logarithm."""
import numpy as np
import pytest

import sample11_cases as sc

F32 = np.float32


@pytest.mark.parametrize("alpha", sc.ALPHAS)
def test_grid_holds_what_it_names(alpha):
    c, s, u1, u2, n_named = sc.grid(alpha)
    assert 2000 < len(c) < 8000 and c.dtype == s.dtype == u1.dtype == u2.dtype == F32
    named = sc.named_cosines()
    side = {k: bool(sc.is_corner(v)) for k, v in named.items()}
    assert side == {"split-4": False, "split-1": False, "split+0": False, "split+1": True, "split+4": True, "zero": False, "nan": False,
                    "+inf": True, "-inf": False}
    # the largest cosine below the split is the split's own literal: the corner is cosTheta > .9999f
    assert named["split+0"] == sc.COS_SPLIT and sc.ulps(sc.COS_SPLIT, 1) > sc.COS_SPLIT
    # every named cosine meets every (U1, U2) pair
    per = len(sc.U1) * len(sc.U2)
    assert n_named == len(named) * per
    for i, v in enumerate(named.values()):
        blk = slice(i * per, (i + 1) * per)
        assert sc.same_bits(c[blk], v).all()
        assert {(a.tobytes(), b.tobytes()) for a, b in zip(u1[blk], u2[blk])} == {(a.tobytes(), b.tobytes()) for a in sc.U1 for b in sc.U2}
    # the roughness moves the stretched cosines: both sides of the split are there without the named ones
    rest = c[n_named:]
    assert sc.is_corner(rest).sum() > 200 and (~sc.is_corner(rest)).sum() > 1000
    assert np.array_equal(s[np.isfinite(c)], sc.sin_of(c[np.isfinite(c)]))
    # U1 and U2 as the issue lists them
    assert [float(x) for x in sc.U1] == [float(x) for x in (F32(0), F32(1e-12), F32(1e-7), sc.ulps(F32(1e-6), -1), F32(1e-6), sc.ulps(F32(1e-6), 1),
                                                               F32(0.25), F32(0.5), sc.ONE_M, F32(1.0))]
    assert [float(x) for x in sc.U2] == [float(x) for x in (F32(0), F32(1e-7), sc.ulps(F32(0.5), -1), F32(0.5), sc.ulps(F32(0.5), 1), sc.ONE_M, F32(1.0))]


@pytest.mark.parametrize("alpha", sc.ALPHAS)
def test_corner_operands_include_the_special_cases_of_the_logarithm(alpha):
    """dm_logf(1 - U1): an ordinary operand, 0 (U1 = 1), a negative one, a NaN and +inf"""
    c, _, u1, _, _ = sc.grid(alpha)
    with np.errstate(invalid="ignore"):
        om = (F32(1) - u1[sc.is_corner(c)]).astype(F32)
    assert ((om > 0) & np.isfinite(om)).sum() > 100
    assert (om == 0).sum() > 10 and (om < 0).sum() > 10 and np.isnan(om).sum() > 10 and (om == np.inf).sum() > 10
    # ... and the Newton lanes' base is 0 (the operand is replaced by 1) and ordinary
    base = F32(1) - np.maximum(u1[~sc.is_corner(c)], F32(1e-6))
    assert (base == 0).sum() > 10 and (base > 0).sum() > 1000


@pytest.mark.parametrize("alpha", sc.ALPHAS)
def test_small_bounds_reach_both_exits_of_the_loop(alpha):
    """the last trip for the second erf_inv is taken by lanes that run out of iterations only: at bound 2 the restated loop must send
    well over the quarter of the Newton inputs there that the GPU test asserts, at bound 3 both exits must be populated, and a wavefront
    of the grid's order must hold both kinds side by side"""
    c, s, u1, _, _ = sc.grid(alpha)
    nw = ~sc.is_corner(c)
    shares = {}
    for cap in (2, 3, 10):
        k = sc.newton_exit(c[nw], s[nw], u1[nw], cap)
        assert set(np.unique(k)) <= {sc.BREAK, sc.RAN_OUT}
        shares[cap] = float((k == sc.RAN_OUT).mean())
    print(alpha, shares)
    assert shares[2] > 0.4 and 0.2 < shares[3] < 0.8 and shares[2] >= shares[3] >= shares[10]
    k2 = np.full(len(c), -1)
    k2[nw] = sc.newton_exit(c[nw], s[nw], u1[nw], 2)
    waves = k2[:len(k2) // sc.WAVE * sc.WAVE].reshape(-1, sc.WAVE)
    mixed = ((waves == sc.BREAK).any(1) & (waves == sc.RAN_OUT).any(1)).sum()
    only_break = ((waves == sc.BREAK).any(1) & ~(waves == sc.RAN_OUT).any(1)).sum()
    assert mixed > 10 and only_break > 0            # the wavefront skips the last trip in some, takes it for a part of its lanes in others


@pytest.mark.parametrize("alpha", sc.ALPHAS)
def test_layouts_are_what_their_names_say(alpha):
    L = sc.layouts(alpha)
    n = len(sc.grid(alpha)[0])
    for name, (fam, c, s, u1, u2) in L.items():
        assert len(fam) == len(c) == len(s) == len(u1) == len(u2) and len(c) % sc.WAVE == 0 and len(c) >= n, name
        assert fam.dtype == np.uint32
    corner = {k: sc.is_corner(v[1]).reshape(-1, sc.WAVE) for k, v in L.items()}
    tr = {k: (v[0] == sc.TR).reshape(-1, sc.WAVE) for k, v in L.items()}
    assert corner["corner_only"].all() and not corner["newton_only"].any()
    assert (corner["both"].any(1) & ~corner["both"].all(1)).all()
    assert not tr["beckmann"].any() and tr["tr"].all() and not tr["both"].any()
    for k in ("corner_only", "newton_only", "both"):
        w = k + "_with_tr"
        assert np.array_equal(corner[w], corner[k])
        assert (tr[w].any(1) & ~tr[w].all(1)).all()
    # beside the Trowbridge-Reitz lanes there are Beckmann lanes of both sides in every wavefront of both_with_tr
    b = ~tr["both_with_tr"]
    assert ((b & corner["both_with_tr"]).any(1) & (b & ~corner["both_with_tr"]).any(1)).all()
    # the whole grid is in `beckmann` and `tr`, in its own order
    assert sc.same_bits(L["beckmann"][1][:n], sc.grid(alpha)[0]).all() and sc.same_bits(L["tr"][3][:n], sc.grid(alpha)[2]).all()
