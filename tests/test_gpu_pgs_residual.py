"""Residual-form motor rows of the one-row-per-lane PGS (pih_wave.h, pgs_rows) against the clamped rows they replace.

pih_config.schedule + 64 switches the speculation off: every env then takes the clamped rows (the z form).  From identical states the two
paths are stepped side by side, with the fp64 oracle as the common reference:
  agreement   both are fp32 roundings of the same solve: the default path's error against the oracle is not larger than the clamped
              path's (p50 and p90 over 256 envs within a factor 1.5, which is what quantiles over 256 envs scatter), same iteration counts;
  fallback    pipe joint speeds of +-300 rad/s make the pipe motors clamp (fp64 oracle with / without the bound: 64 of 64 such envs differ;
              +-20 rad/s: 0 of 64; +-50 / +-100: 18 / 38 of 64, so 20 and 300 are the two values clear of the boundary): the verification must
              fail, the solve is run again with the clamped rows (PIH_S_SOLVER = 4) and the result is the clamped path's bit for bit;
  non-finite  a NaN in one pipe joint velocity: the env is reset, counted and reported as under schedule + 64, the others do not notice;
  scripted    weld rows, clamping arm motors (variant 2: every arm limit row beside residual pipe rows), 40 free-running steps."""
import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import parity_util as P

pytestmark = pytest.mark.gpu

N, PREROLL, SEED = 256, 150, 5
NOSPEC = 1 + 64                                   # schedule: longest-job-first (the default) + no speculation
PV = P.POS + P.VEL                                # position and velocity words of the state record
NOT_SOLVER = [w for w in range(_lib.STATE_WORDS) if w != _lib.S_SOLVER]
QDJ = slice(_lib.S_QDJ, _lib.S_QDJ + 23)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.fixture(scope="module")
def rolled(torch_mod, oracle_mod):
    """256 envs pre-rolled 150 random-action steps on the oracle; the product on both paths synchronised to it, then one step of all three.
    Computed once, read by the tests below."""
    A = oracle_mod.Oracle(N, omp=True, seed=SEED)
    rng = np.random.default_rng(8)
    for _ in range(PREROLL):
        A.step(rng.uniform(-1, 1, (N, 4)))
    gd = P.GpuProduct(N, seed=SEED); gn = P.GpuProduct(N, seed=SEED, schedule=NOSPEC)
    assert gd.cfg.schedule == 1 and gn.cfg.schedule == NOSPEC
    P.sync_product(gd, A); P.sync_product(gn, A)
    before = gd.get_state()
    np.testing.assert_array_equal(before[:, :_lib.S_TIP], gn.get_state()[:, :_lib.S_TIP])
    a = rng.uniform(-1, 1, (N, 4))
    A.step(a); gd.step(a); gn.step(a)
    return dict(before=before, action=a, oracle=A.get_state(), default=gd.get_state(), nospec=gn.get_state())


def _quantile_rule(name, ed, en):
    qd, qn = np.percentile(ed, [50, 90]), np.percentile(en, [50, 90])
    print("%s: error against the fp64 oracle, default path p50 / p90 = %.3e / %.3e ; schedule + 64 path p50 / p90 = %.3e / %.3e" % (name, qd[0], qd[1], qn[0], qn[1]))
    assert qd[0] <= 1.5 * qn[0] and qd[1] <= 1.5 * qn[1], (qd, qn)


def test_agreement_with_the_clamped_rows(rolled):
    so, sd, sn = rolled["oracle"], rolled["default"], rolled["nospec"]
    vd, vn = sd[:, _lib.S_SOLVER].astype(int), sn[:, _lib.S_SOLVER].astype(int)
    print("solver variants: default path %s, schedule + 64 path %s" % (np.bincount(vd, minlength=6).tolist(), np.bincount(vn, minlength=6).tolist()))
    for v in (1, 2, 5):
        assert (vd == v).any(), "variant %d did not occur" % v
    np.testing.assert_array_equal(sd[:, _lib.S_NCONTACT], sn[:, _lib.S_NCONTACT])
    _quantile_rule("one step, 256 envs", np.abs(sd[:, PV] - so[:, PV]).max(1), np.abs(sn[:, PV] - so[:, PV]).max(1))
    differ = sd[:, _lib.S_PGS_ITERS] != sn[:, _lib.S_PGS_ITERS]
    print("PGS iterations differ between the paths in %d of %d envs" % (differ.sum(), N))
    assert differ.mean() < 5e-3                   # the share tests/parity_util.py defaults_one_step_check accepts against the same-cadence oracle
    two = vd == 5                                 # the two-rows-per-lane solver is not touched: the same on both paths
    np.testing.assert_array_equal(sd[two][:, NOT_SOLVER], sn[two][:, NOT_SOLVER])


@pytest.fixture(scope="module")
def pair64(torch_mod, rolled):
    """64-env products on both paths and a function that steps both from the same state"""
    gd = P.GpuProduct(64, seed=SEED); gn = P.GpuProduct(64, seed=SEED, schedule=NOSPEC)

    def run(state):
        out = []
        for g in (gd, gn):
            g.set_state(state)
            o, r, d = g.step(rolled["action"][:64])
            out.append(dict(state=g.get_state(), obs=o, reward=r, done=np.asarray(d), invalid=g.env.invalid().cpu().numpy()))
        return out
    return run


def _with_pipe_speed(rolled, speed):
    s = rolled["before"][:64].copy()
    s[:, QDJ] = speed * np.where(np.arange(23) % 2 == 0, 1.0, -1.0)
    return s


def test_fallback_is_the_clamped_solve_bit_for_bit(rolled, pair64):
    d, n = pair64(_with_pipe_speed(rolled, 300.0))
    vd, vn = d["state"][:, _lib.S_SOLVER].astype(int), n["state"][:, _lib.S_SOLVER].astype(int)
    rows = np.isin(vn, (1, 2, 4))                 # envs the one-row-per-lane solver ran on
    print("+-300 rad/s: default path variants %s, schedule + 64 path %s" % (np.bincount(vd, minlength=6).tolist(), np.bincount(vn, minlength=6).tolist()))
    assert rows.sum() >= 16
    assert (vd[rows] == 4).all() and (vd[~rows] == vn[~rows]).all()
    np.testing.assert_array_equal(d["state"][:, NOT_SOLVER], n["state"][:, NOT_SOLVER])
    for k in ("obs", "reward", "done"):
        np.testing.assert_array_equal(d[k], n[k])


def test_no_fallback_below_the_bound(rolled, pair64):
    d, n = pair64(_with_pipe_speed(rolled, 20.0))
    vd, vn = d["state"][:, _lib.S_SOLVER].astype(int), n["state"][:, _lib.S_SOLVER].astype(int)
    print("+-20 rad/s: default path variants %s, schedule + 64 path %s" % (np.bincount(vd, minlength=6).tolist(), np.bincount(vn, minlength=6).tolist()))
    assert not ((vd == 4) & (vn != 4)).any()
    assert np.isin(vd, (1, 2)).any()              # (the residual rows did run)


def test_non_finite_pipe_velocity(rolled, pair64):
    clean = rolled["before"][:64].copy()
    ref, _ = pair64(clean)
    e = int(np.flatnonzero(np.isin(ref["state"][:, _lib.S_SOLVER].astype(int), (1, 2)))[0])      # an env the residual rows ran on
    bad = clean.copy(); bad[e, _lib.S_QDJ + 11] = np.nan
    d, n = pair64(bad)
    assert np.isfinite(d["state"]).all()
    print("NaN env %d: PIH_S_SOLVER default path %d, schedule + 64 path %d" % (e, d["state"][e, _lib.S_SOLVER], n["state"][e, _lib.S_SOLVER]))
    # the env is reset, counted and reported on both paths: the velocity clamp of the step's tail passes a non-finite value on to the
    # finiteness test (it used to answer a NaN with a bound, and the env went on with +-100 rad/s).  The reset clears PIH_S_SOLVER, so
    # which rows ran is no longer visible in the record; that the speculation cannot accept the NaN shows in the equality with the
    # schedule + 64 path below
    for x in (d, n):
        assert x["state"][e, _lib.S_SPARE] == ref["state"][e, _lib.S_SPARE] + 1 and x["done"][e] == 1 and x["invalid"][e] and x["state"][e, _lib.S_DONE] == 1
        assert x["state"][e, _lib.S_STEPS] == 0 and x["state"][e, _lib.S_SOLVER] == 0
    others = np.arange(64) != e
    np.testing.assert_array_equal(d["state"][others], ref["state"][others])
    for k in ("obs", "reward", "done"):
        np.testing.assert_array_equal(d[k][others], ref[k][others])
    # the env itself: reset, counted (SPARE) and reported (done, invalid) exactly as on the clamped path
    np.testing.assert_array_equal(d["state"][e][NOT_SOLVER], n["state"][e][NOT_SOLVER])
    for k in ("obs", "reward", "done", "invalid"):
        np.testing.assert_array_equal(d[k][e], n[k][e])
    assert d["state"][e, _lib.S_SPARE] == n["state"][e, _lib.S_SPARE]


def test_scripted_mode(torch_mod, oracle_mod):
    kw = dict(mode=1, dv=0.05)
    n = 64
    o = oracle_mod.Oracle(n, omp=True, seed=SEED, **kw)
    gd = P.GpuProduct(n, seed=SEED, **kw); gn = P.GpuProduct(n, seed=SEED, schedule=NOSPEC, **kw)
    P.sync_product(gd, o); P.sync_product(gn, o)
    a = np.zeros((n, 4))
    seen = np.zeros(6, int)
    for _ in range(40):
        o.step(a); gd.step(a); gn.step(a)
        seen += np.bincount(gd.get_state()[:, _lib.S_SOLVER].astype(int), minlength=6)
    print("scripted mode, 64 envs x 40 steps: default path variants %s" % seen.tolist())
    assert seen[2] + seen[5] > 0
    assert seen[4] == 0                           # the verification passed in every env-step: what is compared below is the residual form
    to = o.tip_pose()
    _quantile_rule("scripted, 40 free-running steps, tip pose", np.abs(gd.env.tip_pose().cpu().numpy() - to).max(1), np.abs(gn.env.tip_pose().cpu().numpy() - to).max(1))
