"""The residual form of a never-clamped Gauss-Seidel row (pih_wave.h, pgs_rows), stated in numpy float64.

z form (what the clamped rows run): lane i carries z_i = lambda_i + rhs_i - dinv_i (A lambda)_i; a row update is
    cand = clamp(z_g);  dl = cand - lambda_g;  lambda_g += dl;  z_i += Bn[g][i] dl  for every i,   Bn[g][i] = [g == i] - dinv_i A[i][g].
Residual form: the lanes of rows whose clamp never acts carry r_i = z_i - lambda_i instead; then
    dl = r_g;  lambda_g += dl;  every lane adds Bn[g][i] dl as before, except the row's own lane: coefficient Bn[g][g] - 1 = -dinv_g A[g][g],
the other rows (contact-like: lower bound 0) keep z in the same vector and are updated as in the z form.  The watch is the largest
|lambda| a residual row has held after any sweep; the speculation "never clamped" holds as long as it stays below the row's bound.
Checked here: the identity (multipliers and z agree), the own-lane coefficient, and that the watch fires when a bound is inside the
range the multiplier visits."""
import numpy as np
import pytest

NROWS, NRES, SWEEPS = 40, 23, 50          # rows 0..22 in residual form (symmetric bounds), rows 23..39 with bounds [0, inf)


def _problem(seed):
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(NROWS, NROWS))
    A = M @ M.T + NROWS * np.eye(NROWS)                  # symmetric positive definite Delassus matrix
    rhs = rng.normal(size=NROWS)
    dinv = 1.0 / np.diag(A)
    Bn = np.eye(NROWS) - dinv[None, :] * A               # Bn[g][i] = [g == i] - dinv_i A[i][g]   (A symmetric)
    return A, rhs * dinv, dinv, Bn


def _bounds(hi_res):
    lo = np.concatenate([-hi_res, np.zeros(NROWS - NRES)])
    hi = np.concatenate([hi_res, np.full(NROWS - NRES, np.inf)])
    return lo, hi


def z_form(rhs, Bn, lo, hi):
    lam = np.zeros(NROWS); z = rhs.copy()
    for _ in range(SWEEPS):
        for g in range(NROWS):
            cand = min(max(z[g], lo[g]), hi[g])
            dl = cand - lam[g]; lam[g] += dl
            z += Bn[g] * dl
    return lam, z


def residual_form(rhs, Bn, lo, hi):
    """rows < NRES never clamp (speculated); returns multipliers, z (= r + lambda on the residual rows) and the watch per residual row"""
    Br = Bn.copy()
    for g in range(NRES):
        Br[g, g] -= 1.0                                  # own-lane coefficient: -dinv A[g][g]
    lam = np.zeros(NROWS); v = rhs.copy()                # v: r on rows < NRES, z on the others (lambda = 0 at the start: r = z)
    watch = np.zeros(NRES)
    for _ in range(SWEEPS):
        for g in range(NROWS):
            if g < NRES:
                dl = v[g]
            else:
                dl = min(max(v[g], lo[g]), hi[g]) - lam[g]
            lam[g] += dl
            v += Br[g] * dl
        watch = np.maximum(watch, np.abs(lam[:NRES]))
    z = v.copy(); z[:NRES] += lam[:NRES]
    return lam, z, watch


@pytest.mark.parametrize("seed", range(4))
def test_residual_rows_equal_z_rows_when_no_bound_acts(seed):
    A, rhs, dinv, Bn = _problem(seed)
    np.testing.assert_allclose(np.diag(Bn)[:NRES] - 1.0, -dinv[:NRES] * np.diag(A)[:NRES], rtol=0, atol=1e-15)
    free, _ = z_form(rhs, Bn, *_bounds(np.full(NRES, np.inf)))
    bound = 10.0 * np.abs(free[:NRES]).max() + 1.0       # far from every multiplier
    lo, hi = _bounds(np.full(NRES, bound))
    lz, zz = z_form(rhs, Bn, lo, hi)
    lr, zr, watch = residual_form(rhs, Bn, lo, hi)
    scale = max(np.abs(lz).max(), np.abs(zz).max())
    assert np.abs(lz - lr).max() <= 1e-12 * scale and np.abs(zz - zr).max() <= 1e-12 * scale
    assert (lz[NRES:] >= 0).all() and (lz[NRES:] == 0).any() and (lz[NRES:] > 0).any()      # the bounded rows did clamp: the mix is exercised
    assert (watch < bound).all()


@pytest.mark.parametrize("seed", range(4))
def test_watch_fires_when_a_bound_is_inside_the_multipliers_range(seed):
    A, rhs, dinv, Bn = _problem(seed)
    lo, hi = _bounds(np.full(NRES, np.inf))
    _, _, free_watch = residual_form(rhs, Bn, lo, hi)
    k = int(np.argmax(free_watch))
    hi_res = np.full(NRES, 10.0 * free_watch.max() + 1.0); hi_res[k] = 0.5 * free_watch[k]
    lo, hi = _bounds(hi_res)
    lz, _ = z_form(rhs, Bn, lo, hi)
    lr, _, watch = residual_form(rhs, Bn, lo, hi)
    assert abs(lz[k]) <= hi_res[k] * (1 + 1e-15)         # the z form clamps the row ...
    assert watch[k] >= hi_res[k]                         # ... and the watch of the residual form says so
    assert (watch[np.arange(NRES) != k] < hi_res[np.arange(NRES) != k]).all()
    assert np.abs(lz - lr).max() > 1e-6                  # (the speculated solve is indeed not the clamped one: it has to be run again)
