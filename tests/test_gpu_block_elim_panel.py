"""The block elimination's panel product in the 4x4x4 form of the FP64 MFMA (block_elim.hpp, CAL_PANEL), through the two hooks
of calico_hip_testing.h that run the header's code on its own.

Panel: one wave, a random 4x4 factor W (entry (l16 & 3, lk) in every lane) against a random 16x4 tile x. The result must be
x Wᵀ entry by entry within γ₄ Σ|aₖbₖ|, γ₄ = 4u / (1 - 4u), u = 2⁻⁵³: the bound of a four-term dot product summed in any order.
The host product and the bound are formed in exact rational arithmetic. Whether the 4x4x4 form is bit-identical to register 0 of
the 16x16x4 product it replaces is printed, not required.

One block: calico_debug_block_elim eliminates a 32x32 SPD block with the header's chief and followers (identity tiles -> L⁻ᵀ,
1 or 3 row tiles of X -> Z = X L⁻ᵀ). Reference: Cholesky, L⁻ᵀ and X L⁻ᵀ in numpy.longdouble (64-bit significand: its own error
is 2⁻¹¹ of a double's and does not show in the figures). Error of a matrix: max |got - ref| / max |ref|. Each of L, Z, L⁻ᵀ must
come within 2x the error the 16x16x4 form of the commit before made on the same inputs (tests/golden/block_elim_parent_errors.json,
recorded by tests/golden/make_block_elim_parent.py with that commit's header): room for another rounding order of the same
roundings, not for a lost digit.
Measured (MI355X): the panel's worst error is 0.344 of the bound and it is bit-identical to register 0 of the 16x16x4 product in
64 of 64 lanes; L, Z, L⁻ᵀ of all four cases have the recorded errors in every digit (condition 1e2: L 1.03e-15, Z 2.6e-15 / 2.7e-15,
L⁻ᵀ 2.4e-15; condition 9.4e7: L 6.4e-13, Z 6.8e-10 / 8.3e-10, L⁻ᵀ 1.06e-9) -- the same FMA chains in the same order, so the
factor 2 is moot here.

Bad pivot: the diagonal entry of column 20 (the first of step 5, steps counted from 0) negated. The header does not patch a bad
pivot: L is NaN from column 20 on, columns 0..19 are those of the intact block, and the call returns."""
import ctypes as C
import functools
import json
import os
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_elim_parent_errors.json")
LD = np.longdouble
MATRICES = ("cond1e2", "cond1e8")
ROW_TILES = (1, 3)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block(name):
    """(D [32][32] SPD, its 2-norm condition number). cond1e2: eigenvalues 1 .. 1e-2 in a random basis. cond1e8: unit diagonal
    (equilibrated), condition about 1e8 -- the upper range of the trajectory's band in tests/test_gpu_observability.py."""
    rng = np.random.default_rng(20251 if name == "cond1e2" else 20258)
    q, _ = np.linalg.qr(rng.standard_normal((32, 32)))
    if name == "cond1e2":
        d = (q * np.logspace(0, -2, 32)) @ q.T
    else:
        d = (q * np.logspace(0, -8.2, 32)) @ q.T
        s = 1.0 / np.sqrt(np.diag(d))
        d = d * s[:, None] * s[None, :]
    d = 0.5 * (d + d.T)
    if name == "cond1e8":
        np.fill_diagonal(d, 1.0)
    d.setflags(write=False)
    return d, float(np.linalg.cond(d))


@functools.lru_cache(maxsize=None)
def rows(n_tiles):
    x = np.random.default_rng(77 + n_tiles).standard_normal((16 * n_tiles, 32))
    x.setflags(write=False)
    return x


# ---- reference: Cholesky, L⁻ᵀ and Z = X L⁻ᵀ of a 32x32 block in long double ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, n_tiles):
    assert np.finfo(LD).nmant >= 63, "numpy.longdouble is no wider than double here: no reference"
    a = block(name)[0].astype(LD)
    n = a.shape[0]
    l = np.zeros((n, n), LD)
    for j in range(n):
        l[j, j] = np.sqrt(a[j, j] - np.dot(l[j, :j], l[j, :j]))
        for i in range(j + 1, n):
            l[i, j] = (a[i, j] - np.dot(l[i, :j], l[j, :j])) / l[j, j]
    inv = np.zeros((n, n), LD)            # L⁻¹ by forward substitution, column by column
    for c in range(n):
        for i in range(c, n):
            inv[i, c] = ((LD(1) if i == c else LD(0)) - np.dot(l[i, c:i], inv[c:i, c])) / l[i, i]
    minv = inv.T.copy()
    z = rows(n_tiles).astype(LD) @ minv
    for m in (l, z, minv):
        m.setflags(write=False)
    return l, z, minv


def run_block(hip, d, x):
    """(L, Z, L⁻ᵀ) of calico_debug_block_elim."""
    n_tiles = x.shape[0] // 16
    d, x = np.ascontiguousarray(d, np.float64), np.ascontiguousarray(x, np.float64)
    l, z, minv = np.empty((32, 32)), np.empty((16 * n_tiles, 32)), np.empty((32, 32))
    rc = hip.debug_block_elim(0, n_tiles, _dp(d), _dp(x), _dp(l), _dp(z), _dp(minv))
    assert rc == 0, rc
    return l, z, minv


def block_errors(hip, name, n_tiles):
    """{"L", "Z", "Minv": max |got - ref| / max |ref|} of one case (also what the fixture records)."""
    got = run_block(hip, block(name)[0], rows(n_tiles))
    out = {}
    for key, g, r in zip(("L", "Z", "Minv"), got, reference(name, n_tiles)):
        assert np.isfinite(g).all(), key
        out[key] = float(np.abs(g.astype(LD) - r).max() / np.abs(r).max())
    return out


def case_key(name, n_tiles):
    return "%s/n%d" % (name, n_tiles)


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_panel_product_layout_and_value(hip):
    rng = np.random.default_rng(4)
    w44, x164 = rng.standard_normal((4, 4)), rng.standard_normal((16, 4))
    lane = np.arange(64)
    l16, lk = lane & 15, lane >> 4
    w = np.ascontiguousarray(w44[l16 & 3, lk])
    x = np.ascontiguousarray(x164[l16, lk])
    out = [np.full(64, np.nan), np.full(64, np.nan)]
    for form in (0, 1):
        assert hip.debug_panel_product(0, form, _dp(w), _dp(x), _dp(out[form])) == 0
    gamma4 = Fraction(4, 2 ** 53) / (1 - Fraction(4, 2 ** 53))
    worst = Fraction(0)
    for n in range(64):
        terms = [Fraction(float(x164[l16[n], k])) * Fraction(float(w44[lk[n], k])) for k in range(4)]
        err, bound = abs(Fraction(float(out[1][n])) - sum(terms)), gamma4 * sum(abs(t) for t in terms)
        worst = max(worst, err / bound)
        assert err <= bound, (n, float(err), float(bound))
    same = int((out[0].view(np.uint64) == out[1].view(np.uint64)).sum())
    print("panel product: worst error %.3f of the bound; 4x4x4 form bit-identical to register 0 of the 16x16x4 product in %d of 64 lanes"
          % (float(worst), same))


@pytest.mark.parametrize("n_tiles", ROW_TILES)
@pytest.mark.parametrize("name", MATRICES)
def test_one_block_against_long_double(name, n_tiles, hip):
    parent = json.load(open(GOLDEN))["errors"][case_key(name, n_tiles)]
    cond = block(name)[1]
    assert (50.0 <= cond <= 200.0) if name == "cond1e2" else (3e7 <= cond <= 3e8), cond
    err = block_errors(hip, name, n_tiles)
    for key in ("L", "Z", "Minv"):
        print("%s n_row_tiles %d (condition %.2e): %-4s error %.3e, the 16x16x4 form's %.3e%s"
              % (name, n_tiles, cond, key, err[key], parent[key], " (identical)" if err[key] == parent[key] else ""))
    for key in ("L", "Z", "Minv"):
        assert err[key] <= 2.0 * parent[key], (key, err[key], parent[key])


def test_bad_pivot_is_not_patched(hip):
    d = block("cond1e2")[0].copy()
    good = run_block(hip, d, rows(1))[0]
    d[20, 20] = -d[20, 20]
    l = run_block(hip, d, rows(1))[0]          # (returns: a NaN is ordinary arithmetic)
    low = np.tril(np.ones((32, 32), bool))
    assert np.array_equal(l[:, :20], good[:, :20])
    assert np.isnan(l[:, 20:][low[:, 20:]]).all()
