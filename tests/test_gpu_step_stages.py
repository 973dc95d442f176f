"""The stages of the peg-in-hole step between collision detection and the solve, and the tail of both tasks' steps, on the GPU: the inputs,
metrics and checks of tests/step_stage_cases.py, which tests/test_step_stages.py runs on the host builds.  One step per launch from
set_state, at most 512 envs per launch.

  * contact-row responses (DBG_DINV) of every collision class against oracle.contact_row_response, within GPU_FACTOR x the fp32 host build's
    MEASURED figures; the same bits in the fused launch, the two-launch step and the fused launch without dispatch order, and with
    solver_path = 1: DBG_DINV is read from the contact records AFTER the solve, so every solver (one row per lane, two rows per lane, DOF
    space with the spill area) must leave the response words of every record intact;
  * free acceleration (DBG_UDOT) over the five rate sets against oracle.free_accel, per DOF group and in force space, the same bits in the
    three launch forms;
  * the tail: velocity clamp, quaternion update, reward / done / auto-reset, maxsteps, frozen envs and the non-finite reset (NaN, +-Inf and
    +-2e15 in every checked word) against the oracle's step and a twin handle's masked reset; the non-finite reset of random-fly in both
    layouts, with poisoned and clean envs in one wavefront.

No file of the reference tree is read here."""
import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import collision_cases as K
from tests import parity_util as P
from tests import step_stage_cases as G
from tests.test_collision_domain import _cfg_kw

pytestmark = pytest.mark.gpu
MAX_ENVS = 512
SCHEDULES = (1, 1 + 8, 0)                                    # fused launch, two-launch step, fused launch with block i = env i
FLY_SCHEDULES = (1, 1 + 8, 1 + 32, 1 + 8 + 32)             # quad / lane layout, IK in controller wavefronts / inside the step wavefront
WELL = P.ConditionedParity.WELL
QUAT_TOL = 1e-6                                              # a dozen fp32 operations on numbers of size 1 (eps = 6e-8)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


class Gpu(P.GpuProduct):
    """GpuProduct with the rest of the host build's surface: reset(mask), get_debug()"""

    def reset(self, mask=None):
        self.env.reset(None if mask is None else self.torch.tensor(np.asarray(mask, dtype=np.uint8)))

    def get_debug(self):
        return self.env.debug().cpu().numpy()


def make(n, **cfg):
    return Gpu(n, **cfg)


def make_fly(schedule):
    def f(n, **cfg):
        cfg.setdefault("max_episode_steps", 480); cfg.setdefault("contact_margin", 0.02)
        return Gpu(n, task_id=1, schedule=schedule, **cfg)
    return f


def gpu_debug(states, cfg, schedule, **kw):
    """float32 debug words [n, DEBUG_WORDS] of one step from `states`"""
    n = len(states)
    assert n <= MAX_ENVS
    g = Gpu(n, seed=5, schedule=schedule, debug=1, **cfg, **kw)
    st = g.get_state(); st[:, :K.WORDS] = states; st[:, _lib.S_CACHE_N] = 0
    g.set_state(st)
    g.step(np.zeros((n, 4)))
    return g.get_debug()


# ------------------------------------------------------------------------------------------------ contact-row responses
_ROWS = {}


def gpu_rows(O, name):
    """RowStats of a class, the launches made once: the first launch form against the oracle, the other forms and solver_path = 1 bit for bit"""
    if name in _ROWS:
        return _ROWS[name]
    cs = K.cases(name)
    st = G.RowStats()
    for key, idx in K.group_by_config(cs).items():
        for lo in range(0, len(idx), MAX_ENVS):
            part = idx[lo:lo + MAX_ENVS]
            states = np.array([cs[i].state for i in part])
            d = gpu_debug(states, _cfg_kw(key), SCHEDULES[0])
            st.merge(G.row_errors(O, states, d.astype(np.float64), "GPU %s" % name))
            bits = G.dinv_bits(d)
            for sched in SCHEDULES[1:]:
                d2 = gpu_debug(states, _cfg_kw(key), sched)
                np.testing.assert_array_equal(d2[:, _lib.DBG_NCONTACT], d[:, _lib.DBG_NCONTACT], err_msg="schedule %d" % sched)
                np.testing.assert_array_equal(G.dinv_bits(d2), bits, err_msg="schedule %d" % sched)
            d2 = gpu_debug(states, _cfg_kw(key), SCHEDULES[0], solver_path=1)
            np.testing.assert_array_equal(d2[:, _lib.DBG_NCONTACT], d[:, _lib.DBG_NCONTACT], err_msg="solver_path 1")
            np.testing.assert_array_equal(G.dinv_bits(d2), bits, err_msg="solver_path 1")
    _ROWS[name] = st
    return st


@pytest.mark.parametrize("name", K.CLASSES)
def test_gpu_rows_against_the_oracle(torch_mod, oracle_mod, name):
    st = gpu_rows(oracle_mod, name)
    host = G.MEASURED["rows"][name]
    print("   GPU class %s: %d rows, largest scaled error %.3e = %.2f x the fp32 host build's %.2e (%s)" % (name, st.rows, st.worst, st.worst / host, host, st.where))
    assert st.skipped <= 1e-3 * st.contacts
    assert st.worst <= G.GPU_FACTOR * host, st.where


def test_gpu_rows_cover_brackets_welds_and_null_rows(torch_mod, oracle_mod):
    """what the GPU runs compared, decided by the reference"""
    tot = G.RowStats()
    for name in K.CLASSES:
        tot.merge(gpu_rows(oracle_mod, name))
    print("   GPU: %d rows, per bracket %s, %d attach / weld rows, %d null rows, %d contacts skipped" % (tot.rows, tot.bracket_rows, tot.weld_rows, tot.null_rows, tot.skipped))
    assert min(tot.bracket_rows) >= 1000 and tot.weld_rows >= 200 and tot.null_rows >= 20


# ------------------------------------------------------------------------------------------------ free acceleration
def test_gpu_free_acceleration_against_the_oracle(torch_mod, oracle_mod):
    sets = G.accel_states()
    allst = np.concatenate([sets[n] for n in G.RATE_SETS])
    udot = None
    for sched in SCHEDULES:
        u = np.concatenate([gpu_debug(allst[lo:lo + MAX_ENVS], {}, sched)[:, _lib.DBG_UDOT:_lib.DBG_UDOT + G.ND] for lo in range(0, len(allst), MAX_ENVS)])
        if udot is None:
            udot = u
        else:
            np.testing.assert_array_equal(u.view(np.int32), udot.view(np.int32), err_msg="schedule %d" % sched)
    acc = {g: 0.0 for g in G.GROUPS}; frc = {g: 0.0 for g in G.FORCE_GROUPS}
    lo = 0
    for name in G.RATE_SETS:
        a, f = G.accel_errors(name, udot[lo:lo + len(sets[name])]); lo += len(sets[name])
        print("   GPU rate set %-6s: %s ; force space %s" % (name, {k: "%.2e" % v for k, v in a.items()}, {k: "%.2e" % v for k, v in f.items()}))
        acc = {g: max(acc[g], a[g]) for g in acc}; frc = {g: max(frc[g], f[g]) for g in frc}
    print("   GPU free acceleration / fp32 host build: %s ; force space %s" % ({g: "%.2e = %.2f x" % (v, v / G.MEASURED["accel"][g]) for g, v in acc.items()},
                                                                                 {g: "%.2e = %.2f x" % (v, v / G.MEASURED["force"][g]) for g, v in frc.items()}))
    for g, v in acc.items():
        assert v <= G.GPU_FACTOR * G.MEASURED["accel"][g], (g, v)
    for g, v in frc.items():
        assert v <= G.GPU_FACTOR * G.MEASURED["force"][g], (g, v)


# ------------------------------------------------------------------------------------------------ the tail, peg-in-hole
@pytest.mark.parametrize("auto", [0, 1])
def test_gpu_tail_velocity_clamp(torch_mod, oracle_mod, auto):
    G.check_clamp(oracle_mod, make, auto, WELL)


@pytest.mark.parametrize("auto", [0, 1])
def test_gpu_tail_quaternion_update(torch_mod, oracle_mod, auto):
    G.check_quat(oracle_mod, make, auto, QUAT_TOL)


@pytest.mark.parametrize("auto", [0, 1])
def test_gpu_tail_reward_and_done(torch_mod, oracle_mod, auto):
    G.check_reward_done(oracle_mod, make, auto, WELL)


@pytest.mark.parametrize("auto", [0, 1])
def test_gpu_tail_maxsteps(torch_mod, oracle_mod, auto):
    G.check_maxsteps(oracle_mod, make, auto)


def test_gpu_tail_frozen_envs(torch_mod, oracle_mod):
    G.check_frozen(oracle_mod, make, WELL)


@pytest.mark.parametrize("auto", [0, 1])
def test_gpu_tail_nonfinite_reset(torch_mod, oracle_mod, auto):
    G.check_nonfinite(oracle_mod, make, auto, n=512)


# ------------------------------------------------------------------------------------------------ the tail, random-fly
@pytest.mark.parametrize("sched", FLY_SCHEDULES)
@pytest.mark.parametrize("auto", [0, 1])
def test_gpu_fly_tail_nonfinite_reset(torch_mod, oracle_mod, auto, sched):
    G.check_fly_nonfinite(oracle_mod, make_fly(sched), auto, n=256)


@pytest.mark.parametrize("sched", FLY_SCHEDULES)
def test_gpu_fly_tail_frozen_envs(torch_mod, oracle_mod, sched):
    G.check_fly_frozen(oracle_mod, make_fly(sched), WELL)
