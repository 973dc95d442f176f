"""The stages of the random-fly step between collision detection and the tail, on the CPU (tests/fly_stage_cases.py): free acceleration
(class V), limit rows (class L) and the motor bound (class M), one step per case, both objects.

  * the oracle's new read-outs (joint-row multipliers, last residual, clamp margin) leave its step bit for bit what it was;
  * the floors of every class, the sensitive share and the sweep counts, from the oracle alone;
  * the fp64 host build of the product source (ABA, impulse-response sweeps, speculated limit rows) within 1e-9 of the oracle (RNEA +
    Cholesky, every row in every sweep) at 1 / 2 / 5 sweeps, in the lane layout (step) and the quad layout (step_quad);
  * the fp32 host build within the MEASURED figures, which bound the GPU build (tests/test_gpu_fly_stages.py)."""
import os
import subprocess

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import fly_stage_cases as G
from tests.emul import emul as E
from tests.test_ik_domain import F32_HOST_MAX_A, F64_TOL as IK_F64_TOL

LAYOUTS = ("lane", "quad")
IK_F32 = G.GPU_FACTOR * F32_HOST_MAX_A["ur5"][(0.5, 20)]      # F_TARGET: the bound of tests/test_gpu_ik.py's in-step reading


@pytest.fixture(scope="module", autouse=True)
def _build(oracle_mod):
    E.build()


def host_step(prec, layout, name, ob, iters):
    """(post-step record, debug words) of one step of the host build from the class's states"""
    c = G.cases(name, ob)
    cfg = dict(G.CFG); dt = cfg.pop("dt")
    e = E.EmulFly(c.n, prec, dt=dt, debug=1, object_id=ob, solver_iters=iters, **cfg)
    e.set_state(c.states)
    if layout == "lane":
        e.step(c.actions)
    else:
        assert e.step_quad(c.actions)[3] == 0, "the four lanes of a quad disagree"
    return e.get_state(), e.get_debug()


@pytest.fixture(scope="module")
def host(oracle_mod):
    """{(prec, layout, class, object, sweeps): figures [n] per name}, computed once"""
    out = {}
    for prec in ("f64", "f32"):
        for layout in LAYOUTS:
            for ob in G.OBJECTS:
                out[prec, layout, "V", ob, 1] = G.udot_errors(ob, host_step(prec, layout, "V", ob, 1)[1])
                for name in G.STEP_CLASSES:
                    for it in G.SHORT + (G.LONG,):
                        out[prec, layout, name, ob, it] = G.step_errors(name, ob, it, *host_step(prec, layout, name, ob, it), tag="%s %s %s object %d, %d sweeps" % (prec, layout, name, ob, it))
    return out


def class_worst(host, prec, name, sensitive, long=False):
    """{figure: largest over layouts, objects and sweeps} on the envs that are / are not sensitive (at LONG sweeps: ill-conditioned)"""
    w = {}
    for layout in LAYOUTS:
        for ob in G.OBJECTS:
            for it in ((1,) if name == "V" else (G.LONG,) if long else G.SHORT):
                s = G.ill_conditioned(name, ob) if long else G.reference(name, ob, it).sensitive
                for k, v in G.worst(host[prec, layout, name, ob, it], s if sensitive else ~s).items():
                    w[k] = max(w.get(k, 0.0), v)
    return w


# ------------------------------------------------------------------------------------------------ the oracle alone
def _rollout(O, read, lib_path=None):
    o = O.FlyOracle(70, seed=7, dt=G.DT, residual_threshold=0.0, auto_reset=1, max_episode_steps=150, lib_path=lib_path)
    rng = np.random.default_rng(0)
    for t in range(120):
        o.step(rng.uniform(-1, 1, (70, 6)))
        if read:
            before = o.get_state()
            rows, res, mar = o.debug_rows(), o.pgs_residual(), o.clamp_margin()
            assert np.isfinite(rows).all() and (res >= 0).all() and (mar >= 0).all()
            np.testing.assert_array_equal(o.get_state(), before)
    return o.get_state()


def test_oracle_readouts_leave_the_step_bit_equal(oracle_mod, tmp_path):
    """seed 7, 70 envs, random actions over auto-resets (the rollout of test_fly_one_step_parity_resynchronised): the state after 120 steps
    has the same bits whether the read-outs are read or not, and the bits of a second build of the oracle, same compiler and flags, with
    the read-outs compiled out of the step (-DPIHO_FLY_NO_READOUTS)"""
    a = _rollout(oracle_mod, False); b = _rollout(oracle_mod, True)
    np.testing.assert_array_equal(a, b)
    src = os.path.dirname(os.path.abspath(oracle_mod.__file__)); bare = str(tmp_path / "libpih_oracle_bare.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-std=c11", "-Wno-unused-function", "-fno-fast-math", "-DPIHO_FLY_NO_READOUTS", "-shared", "-o", bare, os.path.join(src, "pih_oracle.c"), "-lm"])
    c = _rollout(oracle_mod, False, lib_path=bare)
    o = oracle_mod.FlyOracle(1, dt=G.DT, lib_path=bare); o.step(np.zeros((1, 6)))
    assert not o.debug_rows().any()                                                  # (the second build does leave them out)
    np.testing.assert_array_equal(a, c)


def test_floors_and_shares_from_the_oracle_alone(oracle_mod):
    lim_dt = G.U_EFFORT * G.DT
    for ob in G.OBJECTS:
        assert (G.reference("V", ob, 1).nc == 0).all()
        cells = G.cell_counts(ob); hist = G.contact_histogram(ob)
        print("   object %d: class N contacts per cell (object / arm-vs-table x depth + slop > 0 / <= 0) %s ; class K cases per contact count %s" % (ob, cells, hist.tolist()))
        assert min(cells) >= 40
        top = G.K_LARGEST[ob]
        assert hist[top] > 0 and not hist[top + 1:].any() and (hist[1:min(top, 10) + 1] >= 5).all()
        if ob == 0:                                                 # (object 1 has two spheres: 2 + 2 + 5 slots, the generator reaches 8)
            assert top >= 12 and hist[G.KR] >= 10 and hist[G.KR + 1] >= 10 and hist[G.KR + 1:].sum() >= 30
            assert hist[G.KR + 1::2].any() and hist[G.KR + 2::2].any()
        else:
            assert hist[G.KR] >= 10
        lim = G.limit_counts(ob); mot = G.motor_counts(ob); free = int(G.motor_only(ob, 5).sum())
        rows = np.abs(G.reference("M", ob, 5).rows[:, :, 0]).max(0)
        print("   object %d: class L active lower / upper multipliers per joint %s ; class M motor rows at -/+ U_EFFORT dt per joint %s (%d in all), largest |motor multiplier| per joint %s of %.2f, %d envs with the motor rows alone" % (
            ob, lim.tolist(), mot.tolist(), mot.sum(), np.round(rows, 3).tolist(), lim_dt[0], free))
        assert lim.min() >= 3
        # The row's multiplier is (KP dq / dt - qd) / W_jj: at the +-90 rad/s of the class, times the reflected inertia of wrist 2 (a few
        # 1e-2 kg m^2) and wrist 3 (4e-3), it stays inside 300 N m x dt = 2.5 N m s; pinned here from the reference
        assert mot.sum() >= 100 and mot[:4].min() >= 1 and free >= 50
        assert rows[5] < 0.5 * lim_dt[5] and (rows[:4] == lim_dt[:4]).all()
        L = G.cases("L", ob); r = G.reference("L", ob, 5)
        fire = (L.kind == G.L_KINDS.index("fire")) & (L.joint < 3)     # (the motor alone stops a wrist joint at 60 rad/s within the step)
        assert (r.rows[fire, L.joint[fire], 1 + L.side[fire]] > 0).all()              # every firing case of the three large joints loads its limit row
        for name in G.STEP_CLASSES:
            for it in G.SHORT:
                r = G.reference(name, ob, it)
                print("   object %d class %s, %d sweeps: %d envs, sensitive share %.4f, sweeps run %s" % (ob, name, it, len(r.sensitive), r.sensitive.mean(), np.bincount(r.iters).tolist()))
                assert r.sensitive.mean() <= G.SENS_SHARE
                assert (r.iters == it).all()
            ill = G.ill_conditioned(name, ob)
            print("   object %d class %s, %d sweeps: ill-conditioned share %.4f" % (ob, name, G.LONG, ill.mean()))
            assert ill.mean() <= G.ILL_SHARE


# ------------------------------------------------------------------------------------------------ host builds of the product source
@pytest.mark.parametrize("name", ("V",) + G.STEP_CLASSES)
def test_f64_host_build_against_the_oracle(host, name):
    w = class_worst(host, "f64", name, False); ws = class_worst(host, "f64", name, True)
    print("   class %s host fp64, both layouts: %s ; sensitive envs %s" % (name, {k: "%.2e" % v for k, v in w.items()}, {k: "%.2e" % v for k, v in ws.items()}))
    for k, v in w.items():
        assert v <= (IK_F64_TOL if k == "target" else G.F64_TOL), (name, k, v)
    for k, v in ws.items():
        assert v <= G.SENS_FACTOR * G.F64_TOL, (name, k, v)


def _hold(name, w, ws, bound):
    for k, v in w.items():
        if k == "target":
            assert v <= IK_F32, (name, v)
            continue
        assert v <= bound[k], (name, k, v)
        assert v >= 0.5 * bound[k], "MEASURED[%s][%s] = %.3e is stale: the build gives %.3e" % (name, k, bound[k], v)
    for k, v in ws.items():
        assert v <= G.SENS_FACTOR * (IK_F32 if k == "target" else bound[k]), (name, k, v)


def test_f32_host_build_within_measured_bounds(host):
    """prints what MEASURED records (pytest -s) and holds the fp32 host build to it; at LONG sweeps the well-conditioned env-steps"""
    w = class_worst(host, "f32", "V", False)
    print("   class V host fp32: %s" % {k: "%.3e" % v for k, v in w.items()})
    _hold("V", w, {}, G.MEASURED["V"])
    for name in G.STEP_CLASSES:
        for long in (False, True):
            w = class_worst(host, "f32", name, False, long); ws = {} if long else class_worst(host, "f32", name, True)
            print("   class %s host fp32, %s: %s" % (name, "%d sweeps" % G.LONG if long else "1 / 2 / 5 sweeps", {k: "%.3e" % v for k, v in w.items()}))
            _hold(name, w, ws, G.MEASURED[name]["long" if long else "short"])
