"""Inputs of sample11 (dev_bsdf.hpp) for tests/test_gpu_sample11_once.py (the device hook trc_sample11_test: the reference's text of
Beckmann's visible-normal sampling against the text that evaluates each exp, log and erf_inv once, TRC_SAMPLE11_ONCE) and
tests/test_sample11_cases.py, which holds this generator to its own conditions on the CPU.

An input is (cosTheta, sinTheta, U1, U2): the cosine and sine of the STRETCHED direction, which is where the roughness enters, and the
two random numbers.  Per roughness there is one grid; layouts() arranges it by wavefront (64 consecutive inputs run as one wavefront of
the hook's kernel) so that the shared logarithm pass and the last trip for the second erf_inv see corner lanes alone, Newton lanes
alone, both, and each of those beside Trowbridge-Reitz lanes.

newton_exit() restates the Newton loop in float32 with numpy's exp / log / arccos in place of trc_detmath.h: good enough to say which
inputs leave the loop by its break and which run out of iterations at a small bound, not to predict bits."""
from collections import OrderedDict

import numpy as np

F32 = np.float32
WAVE = 64
COS_SPLIT = F32(0.9999)              # sample11's corner is cosTheta > .9999f
ALPHAS = (0.01, 0.02, 0.1)           # alpha_y; alpha_x is 0.01 for every lobe
CORNER, BREAK, RAN_OUT, CLOSED_FORM = 0, 1, 2, 3      # the hook's exit kinds
BECKMANN, TR = 0, 1


def ulps(x, k):
    return (np.array(x, F32).view(np.int32) + np.int32(k)).view(F32)[()]


ONE_M = ulps(F32(1.0), -1)
U1 = [F32(0), F32(1e-12), F32(1e-7), ulps(F32(1e-6), -1), F32(1e-6), ulps(F32(1e-6), 1), F32(0.25), F32(0.5), ONE_M, F32(1.0)]
U2 = [F32(0), F32(1e-7), ulps(F32(0.5), -1), F32(0.5), ulps(F32(0.5), 1), ONE_M, F32(1.0)]
# beyond [0, 1]: the remaining special operands of the corner's dm_logf(1 - U1) -- negative, NaN, +inf
U1_EXTRA = [F32(1.5), F32(np.nan), F32(-np.inf)]


def sin_of(cos):
    """sin_theta of the kernels: sqrt(max(0, 1 - z * z)) in float32"""
    cos = np.asarray(cos, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(np.maximum(F32(0), F32(1) - cos * cos)).astype(F32)


def named_cosines():
    """name -> cosTheta: the split's neighbourhood and the operands that are no cosine"""
    d = OrderedDict()
    for k in (-4, -1, 0, 1, 4):
        d[f"split{k:+d}"] = ulps(COS_SPLIT, k)
    d["zero"] = F32(0)
    d["nan"] = F32(np.nan)
    d["+inf"] = F32(np.inf)
    d["-inf"] = F32(-np.inf)
    return d


def stretched_cosines(alpha_y):
    """cosines of directions (theta, phi) stretched by (0.01, alpha_y) and normalised, in float32: theta from the normal to the horizon"""
    theta = np.array([0.05, 0.4, 0.8, 0.9553, 1.2, 1.4, 1.5, 1.55, 1.565, 1.57, 1.5705, 1.5707, 1.57079], np.float64)
    phi = np.array([0.0, 0.7, np.pi / 2], np.float64)
    t, p = np.meshgrid(theta, phi, indexing="ij")
    x, y, z = (F32(0.01) * (np.sin(t) * np.cos(p)).astype(F32), F32(alpha_y) * (np.sin(t) * np.sin(p)).astype(F32), np.cos(t).astype(F32))
    return (z / np.sqrt(x * x + y * y + z * z, dtype=F32)).astype(F32).reshape(-1)


_GRID = {}


def grid(alpha_y):
    """(cos, sin, u1, u2, n_named): every cosine with every (U1, U2) pair, the named cosines first; then the extra U1 on every cosine"""
    if alpha_y not in _GRID:
        named = np.array(list(named_cosines().values()), F32)
        cos = np.concatenate([named, stretched_cosines(alpha_y)])
        uu = np.array([(a, b) for a in U1 for b in U2], F32)
        extra = np.array([(a, b) for a in U1_EXTRA for b in (F32(0.3), F32(0), ONE_M)], F32)
        c = np.concatenate([np.repeat(cos, len(uu)), np.repeat(cos, len(extra))])
        u = np.concatenate([np.tile(uu, (len(cos), 1)), np.tile(extra, (len(cos), 1))])
        out = (c, sin_of(c), np.ascontiguousarray(u[:, 0]), np.ascontiguousarray(u[:, 1]), len(named) * len(uu))
        for a in out[:4]:
            a.setflags(write=False)
        _GRID[alpha_y] = out
    return _GRID[alpha_y]


def is_corner(cos):
    with np.errstate(invalid="ignore"):
        return np.asarray(cos, F32) > COS_SPLIT


def _cycle(idx, n):
    return idx[np.arange(n) % len(idx)]


def layouts(alpha_y):
    """name -> (family, cos, sin, u1, u2), whole wavefronts.  `beckmann` / `tr`: the grid in its own order, one family.  `corner_only`,
    `newton_only`: Beckmann lanes of one side of the split; `both`: even lanes corner, odd lanes Newton.  `*_with_tr`: those three with
    every third lane a Trowbridge-Reitz lane (on the same input the Beckmann lane would have had)."""
    c, s, u1, u2, _ = grid(alpha_y)
    n = -(-len(c) // WAVE) * WAVE
    corner, newton = np.flatnonzero(is_corner(c)), np.flatnonzero(~is_corner(c))
    lane = np.arange(n) % WAVE
    both = np.where(lane % 2 == 0, _cycle(corner, n), _cycle(newton, n))
    every = _cycle(np.arange(len(c)), n)
    third = np.where(lane % 3 == 1, TR, BECKMANN).astype(np.uint32)
    zero = np.zeros(n, np.uint32)
    out = OrderedDict()
    for name, idx, fam in (("beckmann", every, zero), ("tr", every, zero + TR),
                           ("corner_only", _cycle(corner, n), zero), ("newton_only", _cycle(newton, n), zero), ("both", both, zero),
                           ("corner_only_with_tr", _cycle(corner, n), third), ("newton_only_with_tr", _cycle(newton, n), third),
                           ("both_with_tr", both, third)):
        out[name] = (fam, c[idx], s[idx], u1[idx], u2[idx])
    return out


# ------------------------------------------------------------------------------------------------------------------ the loop, restated
def _erf_inv(x):
    x = np.clip(x, F32(-.99999), F32(.99999))
    w = -np.log((F32(1) - x) * (F32(1) + x)).astype(F32)
    lo = w < 5
    wl = w - F32(2.5)
    p = np.full_like(x, F32(2.81022636e-08))
    for k in (3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087, -0.00125372503, -0.00417768164, 0.246640727, 1.50140941):
        p = F32(k) + p * wl
    wh = np.sqrt(np.maximum(w, F32(0))).astype(F32) - F32(3)
    q = np.full_like(x, F32(-0.000200214257))
    for k in (0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773, -0.0076224613, 0.00943887047, 1.00167406, 2.83297682):
        q = F32(k) + q * wh
    return (np.where(lo, p, q) * x).astype(F32)


def _erf_approx(x):
    sign = np.where(x < 0, F32(-1), F32(1))
    x = np.abs(x)
    t = F32(1) / (F32(1) + F32(0.3275911) * x)
    poly = ((((F32(1.061405429) * t + F32(-1.453152027)) * t) + F32(1.421413741)) * t + F32(-0.284496736)) * t + F32(0.254829592)
    return (sign * (F32(1) - poly * t * np.exp(-x * x).astype(F32))).astype(F32)


def newton_exit(cos, sin, u1, cap):
    """exit kind (BREAK or RAN_OUT) of the Newton branch of Beckmann's sample11 per input, with the loop bounded by `cap`"""
    cos, sin, u1 = (np.asarray(a, F32) for a in (cos, sin, u1))
    with np.errstate(all="ignore"):
        tan = (sin / cos).astype(F32)
        cot = (F32(1) / tan).astype(F32)
        a = np.full_like(cos, F32(-1))
        c = _erf_approx(cot)
        sample_x = np.where(u1 > F32(1e-6), u1, F32(1e-6)).astype(F32)          # fmaxf: a NaN gives the other operand
        theta = np.arccos(np.clip(cos, F32(-1), F32(1))).astype(F32)
        fit = F32(1) + theta * (F32(-0.876) + theta * (F32(0.4265) - F32(0.0594) * theta))
        base = F32(1) - sample_x
        pw = np.exp(fit * np.log(np.where(base == 0, F32(1), base)).astype(F32)).astype(F32)
        b = c - (F32(1) + c) * np.where(base == 0, F32(0), pw)
        spi = F32(1.0 / np.sqrt(np.pi))
        norm = F32(1) / (F32(1) + c + spi * tan * np.exp(-cot * cot).astype(F32))
        live = np.ones(len(cos), bool)
        kind = np.full(len(cos), RAN_OUT, np.int32)
        it = 0
        while True:
            it += 1
            if not it < cap:
                break
            b = np.where(live & ~((b >= a) & (b <= c)), F32(0.5) * (a + c), b).astype(F32)
            inv = _erf_inv(b)
            value = norm * (F32(1) + b + spi * tan * np.exp(-inv * inv).astype(F32)) - sample_x
            deriv = norm * (F32(1) - inv * tan)
            done = live & (np.abs(value) < F32(1e-5))
            kind[done] = BREAK
            live &= ~done
            c = np.where(live & (value > 0), b, c).astype(F32)
            a = np.where(live & ~(value > 0), b, a).astype(F32)
            b = np.where(live, b - value / deriv, b).astype(F32)
    return kind


def same_bits(a, b):
    """elementwise: the same bit pattern, or both NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
