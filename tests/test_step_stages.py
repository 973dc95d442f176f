"""The stages of the peg-in-hole step between collision detection and the solve, and the step's tail, on the CPU (tests/step_stage_cases.py):

  * the oracle's stand-alone contact-row primitive gives, bit for bit, the rows of its own step (one shared row function);
  * the fp64 host build of the product source (ABA response sweeps) stays within 1e-9 of the oracle (RNEA + Cholesky) on the contact-row
    responses of every collision class and on the free acceleration of every rate set: two independent algorithms pinned to each other;
  * the fp32 host build stays within the MEASURED figures, which bound the GPU build (tests/test_gpu_step_stages.py);
  * the tail (velocity clamp, quaternion update, reward / done, maxsteps, frozen envs, non-finite reset) of the fp64 host build against the
    oracle, with the case generators of the GPU tests: a disagreement there is then in the wave layer, not in the algorithm."""
import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import collision_cases as K
from tests import step_stage_cases as G
from tests.emul import emul as E
from tests.test_collision_domain import _cfg_kw

F64_TAIL = 1e-9      # free flight: two fp64 algorithms agree to rounding
F64_QUAT = 1e-13     # the quaternion update: a dozen fp64 operations on numbers of size 1 (eps = 1.1e-16), two orders of room
F64_SOLVE = 1e-6     # where 50 PGS sweeps act on fast or contacting states: the bound of test_emul_parity's one-step equivalence


@pytest.fixture(scope="module", autouse=True)
def _build(oracle_mod):
    E.build()


def host_debug(prec, states, cfg):
    """debug words [n, DEBUG_WORDS] of one step of the host build from `states`"""
    e = E.Emul(len(states), prec, debug=1, **cfg)
    s = e.get_state(); s[:, :K.WORDS] = states; s[:, _lib.S_CACHE_N] = 0
    e.set_state(s)
    e.step(np.zeros((len(states), 4)))
    return e.get_debug()


@pytest.fixture(scope="module")
def host_rows(oracle_mod):
    """{(prec, class): RowStats}, computed once"""
    out = {}
    for prec in ("f64", "f32"):
        for name in K.CLASSES:
            cs = K.cases(name); st = G.RowStats()
            for key, idx in K.group_by_config(cs).items():
                states = np.array([cs[i].state for i in idx])
                st.merge(G.row_errors(oracle_mod, states, host_debug(prec, states, _cfg_kw(key)), "%s %s" % (prec, name)))
            out[prec, name] = st
    return out


@pytest.fixture(scope="module")
def host_accel():
    """{(prec, rate set): (group figures, force-space figures)}"""
    return {(prec, name): G.accel_errors(name, host_debug(prec, s, {})[:, _lib.DBG_UDOT:_lib.DBG_UDOT + G.ND]) for prec in ("f64", "f32") for name, s in G.accel_states().items()}


def make_f64(n, **cfg):
    return E.Emul(n, "f64", **cfg)


# ------------------------------------------------------------------------------------------------ the oracle's primitive
def test_primitive_equals_the_rows_of_the_oracles_step(oracle_mod):
    """piho_step and piho_contact_row_response share one row function: on the oracle's own contact list the primitive returns the step's
    J M^-1 J^T bit for bit (every class; attach and weld rows, spill-sized lists)"""
    O = oracle_mod
    rows = 0
    for name in K.CLASSES:
        cs = K.cases(name)[::4]
        for key, idx in K.group_by_config(cs).items():
            o = O.Oracle(len(idx), **_cfg_kw(key))
            s = o.get_state(); s[:, :K.WORDS] = [cs[i].state for i in idx]; o.set_state(s)
            s = o.get_state()
            o.step(np.zeros((len(idx), 4)))
            con, cnt = o.debug_contacts_all()
            for e in range(len(idx)):
                c = con[e, :cnt[e]]
                if cnt[e]:
                    jw = O.contact_row_response(s[e], c[:, 0].astype(np.int32), c[:, 1].astype(np.int32), c[:, 2:5], c[:, 5:8], c[:, 9])
                    np.testing.assert_array_equal(jw, o.debug_row_jw(e)[:cnt[e]])
                    rows += 3 * cnt[e]
    assert rows > 10000


def test_rows_cover_brackets_welds_and_null_rows(host_rows):
    """from the reference alone: every contact-count bracket, the attach / weld rows and the null friction rows are compared; at most
    0.1 % of a class's contacts lose their friction rows to the tangent-branch edge"""
    for prec in ("f64", "f32"):
        tot = G.RowStats()
        for name in K.CLASSES:
            st = host_rows[prec, name]; tot.merge(st)
            assert st.skipped <= 1e-3 * st.contacts, (prec, name, st.skipped, st.contacts)
        print("   %s: %d rows, per bracket %s, %d attach / weld rows, %d null rows, %d contacts skipped" % (prec, tot.rows, tot.bracket_rows, tot.weld_rows, tot.null_rows, tot.skipped))
        assert min(tot.bracket_rows) >= 1000 and tot.weld_rows >= 200 and tot.null_rows >= 20


@pytest.mark.parametrize("name", K.CLASSES)
def test_f64_host_build_rows_against_the_oracle(host_rows, name):
    st = host_rows["f64", name]
    print("   class %s host fp64: %d rows, largest scaled error %.3e (%s)" % (name, st.rows, st.worst, st.where))
    assert st.worst <= G.F64_TOL, st.where


@pytest.mark.parametrize("name", G.RATE_SETS)
def test_f64_host_build_free_acceleration_against_the_oracle(host_accel, name):
    acc, frc = host_accel["f64", name]
    print("   rate set %s host fp64: %s ; force space %s" % (name, {k: "%.2e" % v for k, v in acc.items()}, {k: "%.2e" % v for k, v in frc.items()}))
    assert max(acc.values()) <= G.F64_TOL and max(frc.values()) <= G.F64_TOL


def test_f32_host_build_within_measured_bounds(host_rows, host_accel):
    """prints what MEASURED records (pytest -s) and holds the fp32 host build to it"""
    rows = {name: host_rows["f32", name].worst for name in K.CLASSES}
    acc = {g: max(host_accel["f32", n][0][g] for n in G.RATE_SETS) for g in G.GROUPS}
    frc = {g: max(host_accel["f32", n][1][g] for n in G.RATE_SETS) for g in G.FORCE_GROUPS}
    print("   fp32 host build rows:  %s" % {k: "%.3e" % v for k, v in rows.items()})
    print("   fp32 host build accel: %s" % {k: "%.3e" % v for k, v in acc.items()})
    print("   fp32 host build force: %s" % {k: "%.3e" % v for k, v in frc.items()})
    for got, key in ((rows, "rows"), (acc, "accel"), (frc, "force")):
        for k, v in got.items():
            assert v <= G.MEASURED[key][k], (key, k, v, host_rows["f32", k].where if key == "rows" else None)
            assert v >= 0.5 * G.MEASURED[key][k], "MEASURED[%s][%s] = %.3e is stale: the build gives %.3e" % (key, k, G.MEASURED[key][k], v)
    # the force-space figure is the tighter one on the groups it is kept for
    assert all(frc[g] < 0.1 * acc[g] for g in G.FORCE_GROUPS)


# ------------------------------------------------------------------------------------------------ the tail, fp64 host build
@pytest.mark.parametrize("auto", [0, 1])
def test_tail_velocity_clamp(oracle_mod, auto):
    G.check_clamp(oracle_mod, make_f64, auto, F64_SOLVE)


@pytest.mark.parametrize("auto", [0, 1])
def test_tail_quaternion_update(oracle_mod, auto):
    G.check_quat(oracle_mod, make_f64, auto, F64_QUAT)


@pytest.mark.parametrize("auto", [0, 1])
def test_tail_reward_and_done(oracle_mod, auto):
    G.check_reward_done(oracle_mod, make_f64, auto, F64_TAIL)


@pytest.mark.parametrize("auto", [0, 1])
def test_tail_maxsteps(oracle_mod, auto):
    G.check_maxsteps(oracle_mod, make_f64, auto)


def test_tail_frozen_envs(oracle_mod):
    G.check_frozen(oracle_mod, make_f64, F64_SOLVE)


@pytest.mark.parametrize("auto", [0, 1])
def test_tail_nonfinite_reset(oracle_mod, auto):
    G.check_nonfinite(oracle_mod, make_f64, auto, n=512)


# ------------------------------------------------------------------------------------------------ the tail of random-fly, fp64 host build
def make_fly_f64(n, **cfg):
    return E.EmulFly(n, "f64", **cfg)


@pytest.mark.parametrize("auto", [0, 1])
def test_fly_tail_nonfinite_reset(oracle_mod, auto):
    G.check_fly_nonfinite(oracle_mod, make_fly_f64, auto)


def test_fly_tail_frozen_envs(oracle_mod):
    G.check_fly_frozen(oracle_mod, make_fly_f64, F64_SOLVE)
