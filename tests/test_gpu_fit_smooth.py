"""The smoothing spline fit on the device (`-m gpu`): calico_fit_spline_smooth against tests/fit_smooth_ref.py (proved on the CPU in
test_fit_smooth_reference.py) over orders, sampling patterns, derivatives and lambdas with seeded weights; what the penalty is for
(the gap); and the contracts of the call: lambda 0 without weights is calico_fit_spline bit for bit, samples of weight 0 are not
read, the groups and the lambdas of a grid do not see each other, the selection rule, determinism and the LDS ceiling.

rss and penalty are held to 1e-12 of the sum of the magnitudes of their terms, not of their value: both cancel (the residual of a
smooth channel is 1e-8 of the data, the penalty of a smoothed one a 1e-5th of its terms), so that the device's own spline weights,
a few ulp from numpy's, already move the value by more than 1e-12 of itself. The sweep prints both ratios."""
import ctypes as C

import numpy as np
import pytest

import fit_ref
import fit_smooth_ref as fs
from calico_amd import _capi

pytestmark = pytest.mark.gpu


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _smooth(hip, c, weights=None, **options):
    o = _capi.default_spline_fit_options(hip, **options) if options else None
    return _capi.fit_spline_smooth(hip, c.order, c.knots, c.basis, c.stamps, c.data, weights, o)


def _plain(hip, c):
    ctrl = np.full((c.n_ctrl, 6), np.nan)
    assert hip.fit_spline(0, c.order, len(c.knots), dp(c.knots), dp(c.basis), len(c.stamps), dp(c.stamps), dp(c.data), dp(ctrl)) == _capi.OK
    return ctrl


def _without(c, keep):
    """Case c with only the samples of `keep` (same knots)."""
    from types import SimpleNamespace
    return SimpleNamespace(order=c.order, n_ctrl=c.n_ctrl, knots=c.knots, basis=c.basis, stamps=np.ascontiguousarray(c.stamps[keep]),
                           data=np.ascontiguousarray(c.data[keep]))


@pytest.mark.parametrize("name,m", list(fs.SWEEP))
def test_smooth_fit_sweep_against_long_double(name, m, hip):
    """Per (group, lambda) of the entry's grid (fit_smooth_ref.check): backward error against A and b in long double <= 1e-11;
    control points and fitted values within 1e-14 cond2(A) max|C_ref| + 1e-13 max|data| of the long-double Cholesky's; the
    absolute lambda within 1e-12; rss and penalty within 1e-12 of their terms of the long-double sums at the device's own
    control points; no replaced pivot."""
    p = fs.problem(name, m)
    out = _smooth(hip, p.c, p.weights, derivative=m, lambda_rot=p.grid[0], lambda_pos=p.grid[1])
    assert out["summary"] == dict(status=[0, 0], chosen=[0, 0], n_used=[len(p.c.stamps)] * 2)
    assert np.array_equal(out["ctrl"], out["ctrl_all"][0])
    result = fs.check(p, out)
    assert not fs.failed(result), result


def test_gap_is_filled_where_the_plain_fit_drops_its_control_points(hip):
    """gap-12-segments: calico_fit_spline leaves the control points the gap does not determine at <= 1e-12 max|data|, as it always
    did; the smoothing fit with its defaults has every one of them above 0.1 max|data|, and meets its reference."""
    c = fit_ref.case("gap-12-segments")
    dropped = ~fit_ref.reference("gap-12-segments").kept
    scale = np.abs(c.data).max()
    assert dropped.sum() >= 5 and np.abs(_plain(hip, c)[dropped]).max() <= fit_ref.DROPPED_BOUND * scale
    out = _smooth(hip, c)
    assert np.abs(out["ctrl"][dropped]).max(1).min() > 0.1 * scale
    p = fs.build(c, np.ones((len(c.stamps), 2)), 2, (1e-3,), (1e-3,))
    result = fs.check(p, out, label=" (defaults)")
    assert not fs.failed(result), result


@pytest.mark.parametrize("name", ["order6-f1", "rough-order6-f0.5", "gap-12-segments", "order8-f0.5"])
def test_lambda_zero_without_weights_is_the_plain_fit_bit_for_bit(name, hip):
    c = fit_ref.case(name)
    out = _smooth(hip, c, lambda_rot=0.0, lambda_pos=0.0)
    plain = _plain(hip, c)
    assert np.array_equal(out["ctrl"], plain) and np.array_equal(out["ctrl_all"][0], plain)
    assert [r[0]["lambda"] for r in out["rows"]] == [0.0, 0.0]
    ones = _smooth(hip, c, np.ones((len(c.stamps), 2)), lambda_rot=0.0, lambda_pos=0.0)      # (w_a (w_b 1): weight 1 changes no bit)
    assert np.array_equal(ones["ctrl"], plain)


def test_samples_of_weight_zero_are_not_read(hip):
    """A tenth of the samples at weight 0 in the rotation column, another tenth in the position column, their channels NaN: each
    group has the bits of the call without its samples, and n_used counts the rest."""
    c = fit_ref.case("rough-order6-f1")
    n = len(c.stamps)
    w = fs.sample_weights(n, seed=5)
    rng = np.random.default_rng(6)
    off = [rng.choice(n, n // 10, replace=False) for _ in range(2)]
    data = c.data.copy()
    for g in range(2):
        w[off[g], g] = 0.0
        data[off[g], 3 * g:3 * g + 3] = np.nan
    from types import SimpleNamespace
    poisoned = SimpleNamespace(order=c.order, n_ctrl=c.n_ctrl, knots=c.knots, basis=c.basis, stamps=c.stamps, data=data)
    out = _smooth(hip, poisoned, w)
    assert out["summary"]["n_used"] == [n - n // 10] * 2 and np.isfinite(out["ctrl"]).all()
    for g in range(2):
        keep = np.setdiff1d(np.arange(n), off[g])
        part = _smooth(hip, _without(c, keep), np.ascontiguousarray(w[keep]))
        assert np.array_equal(out["ctrl"][:, 3 * g:3 * g + 3], part["ctrl"][:, 3 * g:3 * g + 3]), g
        # (the row too, but for rss: its 64 lanes stride over the samples' indices, so leaving samples out regroups the sum)
        a, b = out["rows"][g][0], part["rows"][g][0]
        assert all(a[k] == b[k] for k in ("status", "replaced_pivots", "lambda", "penalty"))
        assert abs(a["rss"] - b["rss"]) <= 1e-14 * b["rss"] and abs(a["rms"] - b["rms"]) <= 1e-14 * b["rms"]


def test_groups_are_independent(hip):
    c = fit_ref.case("rough-order6-f1")
    w = fs.sample_weights(len(c.stamps))
    grid = (1e-4, 1e-2)
    a = _smooth(hip, c, w, lambda_rot=grid, lambda_pos=grid)
    w2 = w.copy()
    w2[:, 1] = w[::-1, 1]
    b = _smooth(hip, c, w2, lambda_rot=grid, lambda_pos=(1e-5, 1.0))
    assert np.array_equal(a["ctrl_all"][:, :, :3], b["ctrl_all"][:, :, :3]) and a["rows"][0] == b["rows"][0]
    assert not np.array_equal(a["ctrl_all"][:, :, 3:], b["ctrl_all"][:, :, 3:])


GRID32 = tuple(10.0 ** np.linspace(-6.0, 0.0, 32))


def test_grid_of_32_lambdas(hip):
    """Every lambda of a 32-entry grid has the bits of its own single-lambda call; an absolute lambda gives the bits of the relative
    one it equals; rss does not decrease and the penalty does not increase along the grid, up to what the forward bound lets
    either move; and the selection rule."""
    p = fs.build(fit_ref.case("rough-order6-f1"), fs.sample_weights(len(fit_ref.case("rough-order6-f1").stamps)), 2, GRID32, GRID32,
                 reference=False)
    c, w = p.c, p.weights
    out = _smooth(hip, c, w, lambda_rot=GRID32, lambda_pos=GRID32)
    assert out["summary"]["status"] == [0, 0] and out["summary"]["chosen"] == [0, 0]
    for l in range(32):
        one = _smooth(hip, c, w, lambda_rot=GRID32[l], lambda_pos=GRID32[l])
        assert np.array_equal(one["ctrl"], out["ctrl_all"][l]), l
        assert [one["rows"][g][0] for g in range(2)] == [out["rows"][g][l] for g in range(2)], l
    absolute = _smooth(hip, c, w, relative=0, lambda_rot=[r["lambda"] for r in out["rows"][0]], lambda_pos=[r["lambda"] for r in out["rows"][1]])
    assert np.array_equal(absolute["ctrl_all"], out["ctrl_all"]) and absolute["rows"] == out["rows"]
    bound = 1e-14 * 1e7 * np.abs(out["ctrl_all"]).max() + 1e-13 * np.abs(c.data).max()      # (cond2 <= 5.6e6 on this case: the sweep's table)
    for g in range(2):
        rows = out["rows"][g]
        sw, n_p = w[:, g].sum(), fs.band_inf_norm(p.P)
        for l in range(31):
            # a move of every fitted value by `bound` moves rss by at most 2 sqrt(rss sum w) bound + sum w bound^2, and a move of
            # every control point moves c'Pc by at most 2 ||P||_inf sum|c| bound (+ second order)
            assert rows[l + 1]["rss"] >= rows[l]["rss"] - (2 * np.sqrt(rows[l]["rss"] * sw) * bound + sw * bound ** 2), (g, l)
            csum = np.abs(out["ctrl_all"][l][:, 3 * g:3 * g + 3]).sum()
            assert rows[l + 1]["penalty"] <= rows[l]["penalty"] + 2 * n_p * csum * bound * 1.01, (g, l)
        assert rows[31]["rss"] > 1.05 * rows[0]["rss"] and rows[31]["penalty"] < 0.01 * rows[0]["penalty"]
    # the discrepancy principle: a target between the rms of rows 24 and 25 (rotation) and of rows 28 and 29 (position)
    rms = [[r["rms"] for r in out["rows"][g]] for g in range(2)]
    assert all(rms[g][l + 1] > rms[g][l] for g in range(2) for l in (24, 28))
    chosen = _smooth(hip, c, w, lambda_rot=GRID32, lambda_pos=GRID32, target_rms_rot=0.5 * (rms[0][24] + rms[0][25]),
                     target_rms_pos=0.5 * (rms[1][28] + rms[1][29]))
    assert chosen["summary"]["status"] == [0, 0] and chosen["summary"]["chosen"] == [24, 28]
    assert np.array_equal(chosen["ctrl"][:, :3], out["ctrl_all"][24][:, :3]) and np.array_equal(chosen["ctrl"][:, 3:], out["ctrl_all"][28][:, 3:])
    missed = _smooth(hip, c, w, lambda_rot=GRID32, lambda_pos=GRID32, target_rms_rot=0.5 * min(rms[0]), target_rms_pos=2.0 * max(rms[1]))
    assert missed["summary"]["status"] == [_capi.FIT_TARGET_NOT_MET, 0] and missed["summary"]["chosen"] == [0, 31]
    assert np.array_equal(missed["ctrl"][:, :3], out["ctrl_all"][0][:, :3]) and np.array_equal(missed["ctrl"][:, 3:], out["ctrl_all"][31][:, 3:])


def test_smooth_fit_is_bit_reproducible(hip):
    p = fs.problem("gap-12-segments", 2)
    a, b = [_smooth(hip, p.c, p.weights, lambda_rot=fs.GRID, lambda_pos=fs.GRID) for _ in range(2)]
    assert np.array_equal(a["ctrl_all"], b["ctrl_all"]) and np.array_equal(a["ctrl"], b["ctrl"]) and a["rows"] == b["rows"]


@pytest.mark.parametrize("n_ctrl", [911, 2218])
def test_lengths_at_the_lds_limits(n_ctrl, hip):
    """Order 6 at the first length above 64 KiB of [band | 3 rhs] (911 x 9 x 8 bytes) and at the 156 KiB ceiling (2218): backward
    error <= 1e-11 against A and b in long double, no replaced pivot."""
    c = fit_ref.inputs(fit_ref._ragged(6, 1.0, n_ctrl, 20.0))
    assert (n_ctrl - 1) * 9 * 8 <= (64 if n_ctrl == 911 else 156) * 1024 < n_ctrl * 9 * 8 + (0 if n_ctrl == 911 else 72)
    p = fs.build(c, fs.sample_weights(len(c.stamps)), 2, (1e-3,), (1e-3,), reference=False)
    out = _smooth(hip, c, p.weights)
    for g in range(2):
        eta = fs.backward_error(p.sys[g, 0].A, p.b[g], out["ctrl"][:, 3 * g:3 * g + 3]).max()
        print("order 6 n_ctrl %d group %d eta %.1e" % (n_ctrl, g, eta))
        assert eta <= fit_ref.ETA_BOUND and out["rows"][g][0]["replaced_pivots"] == 0 and out["rows"][g][0]["status"] == 0


def test_one_control_point_past_the_ceiling_is_refused(hip):
    c = fit_ref.inputs(fit_ref._ragged(6, 1.0, 2219, 20.0))
    ctrl, summary = np.full((c.n_ctrl, 6), 7.5), _capi.SplineFitSummary()
    rc = hip.fit_spline_smooth(0, c.order, len(c.knots), dp(c.knots), dp(c.basis), len(c.stamps), dp(c.stamps), dp(c.data), None, None, dp(ctrl),
                               None, None, C.byref(summary))
    assert rc == _capi.UNIMPLEMENTED and (ctrl == 7.5).all()
    assert hip.last_error(None).decode().startswith("calico_fit_spline_smooth: ")
