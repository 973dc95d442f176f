"""GPU parity tests proper: the HIP path, called through the C ABI (include/pih.h), against the fp64 oracle on the same
seeded inputs.  Tolerance (north_star): peg-tip pose 1e-3 m, contact-normal force 1e-2 N over 1000 steps on contact-stable
scenarios; chaotic phases are compared one step at a time from a resynchronised state.  PARITY UNPINNED vs PyBullet."""
import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import parity_util as P
from tests import step_stage_cases as G

pytestmark = pytest.mark.gpu

REST = np.array([0, -0.215, -np.pi / 3, -2.57, 0, 2.356, 2.356, 0, 0])
POS = [*range(_lib.S_QARM, _lib.S_QDARM), *range(_lib.S_POS, _lib.S_VLIN), *range(_lib.S_QJ, _lib.S_QDJ)]
VEL = [*range(_lib.S_QDARM, _lib.S_POS), *range(_lib.S_VLIN, _lib.S_QJ), *range(_lib.S_QDJ, _lib.S_TARGET)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


def _gpu(n, **kw):
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    return PihVecEnv(n, **kw)


def _to_gpu_state(torch, env, s98):
    st = env.state().cpu().numpy().astype(np.float64)
    st[:, :_lib.S_TIP] = s98[:, :_lib.S_TIP]
    st[:, _lib.S_CACHE_N] = 0
    env.set_state(torch.tensor(st, dtype=torch.float32))


def test_native_library_loaded(torch_mod):
    import ctypes
    L = _lib.load()
    assert isinstance(L, ctypes.CDLL) and L.pih_abi_version() == 4


def test_reset_matches_oracle(torch_mod, oracle_mod):
    g = _gpu(256, seed=3)
    o = oracle_mod.Oracle(256, seed=3)
    sg = g.state().cpu().numpy()
    np.testing.assert_allclose(sg[:, :_lib.S_TIP], o.get_state()[:, :_lib.S_TIP], atol=1e-6)
    np.testing.assert_allclose(g.tip_pose().cpu().numpy(), o.tip_pose(), atol=1e-6)


def test_ik_matches_oracle(torch_mod, oracle_mod):
    torch = torch_mod
    rng = np.random.default_rng(0)
    n = 64
    tq = oracle_mod.quat_from_euler([0, -np.pi, 0])
    q0 = np.tile(REST, (n, 1)); q0[:, :7] += rng.uniform(-0.3, 0.3, (n, 7))
    tgt = np.array([oracle_mod.fk_arm(q, 9)[0] for q in q0]) + rng.uniform(-0.02, 0.02, (n, 3))
    ref = np.array([oracle_mod.ik(q0[i], tgt[i], tq) for i in range(n)])
    g = _gpu(1)
    out = g.ik(torch.tensor(q0), torch.tensor(tgt), torch.tensor(np.tile(tq, (n, 1)))).cpu().numpy()
    np.testing.assert_allclose(out, ref, atol=3e-5)


def test_one_step_parity_resynchronised(torch_mod, oracle_mod):
    """Random-action rollout, GPU state overwritten with the oracle's before every step (so chaos cannot amplify).
    Contact sets, done flags and the free acceleration must agree always; pose / force errors are bounded on EVERY env-step: within
    1e-4, or within 10 x what the fp64 oracle itself does under 1e-6 perturbations of that step's input (tests/parity_util.py
    ConditionedParity: a loaded mu = 10 tip contact under fast motion is ill-posed for 50 PGS sweeps in any precision)."""
    torch = torch_mod
    N = 32
    o = oracle_mod.Oracle(N, residual_threshold=0.0, warmstart=0.0)
    led = P.ConditionedParity(oracle_mod, with_cache=False, slots=128, residual_threshold=0.0, warmstart=0.0)
    g = _gpu(N, residual_threshold=0.0, warmstart=0.0, debug=1)
    rng = np.random.default_rng(0)
    perr, ferr = [], []
    hist = np.zeros(49, int)
    accel = {grp: 0.0 for grp in G.GROUPS}
    for t in range(300):
        a = rng.uniform(-1, 1, (N, 4))
        _to_gpu_state(torch, g, o.get_state()); led.before(o)
        oo, ro, do = o.step(a)
        np.add.at(hist, o.ncontacts(), 1)
        og, rg, dg = g.step(torch.tensor(a, dtype=torch.float32))
        so = o.get_state(); sg = g.state().cpu().numpy().astype(np.float64)
        ud = np.array([o.debug_udot(i) for i in range(N)])
        dbg = g.debug().cpu().numpy()
        assert (np.abs(ud - dbg[:, _lib.DBG_UDOT:_lib.DBG_UDOT + 38]).max(1) <= 1e-3 * (1 + np.abs(ud).max(1))).all()     # free acceleration, fp32
        for grp, fig in G.accel_group_metric(dbg[:, _lib.DBG_UDOT:_lib.DBG_UDOT + 38], ud).items():               # ... per DOF group: a pipe joint's 1e6 rad/s^2 does not hide the arm
            accel[grp] = max(accel[grp], fig)
            assert fig <= G.GPU_FACTOR * G.MEASURED["accel"][grp], (t, grp, fig)
        np.testing.assert_array_equal(o.ncontacts(), sg[:, _lib.S_NCONTACT].astype(int))               # same contact sets
        np.testing.assert_array_equal(dg.cpu().numpy(), do)
        np.testing.assert_allclose(og.cpu().numpy()[:, 2:], oo[:, 2:], atol=1e-4)          # ee position
        perr.append(np.abs(so[:, POS] - sg[:, POS]).max(1))
        cf = o.contact_force(); ferr.append(np.abs(sg[:, _lib.S_CFORCE] - cf) / (1 + np.abs(cf)))
        led.after(o, a, perr[-1], ferr[-1])
    print("contact-count histogram (env-steps per count):", hist[:hist.nonzero()[0].max() + 1].tolist())
    print("free acceleration per DOF group, max|err| / (1 + max|ref|):", {k: "%.2e" % v for k, v in accel.items()})
    # both sides of the merged first response pass (MERGED_CONTACTS = 10: <= 10 contacts take one sweep, 11 take two)
    assert hist[10] > 20 and hist[11] > 20 and hist[9] > 20 and hist[12] > 20
    led.finish("one-step resynchronised N=32")


@pytest.mark.parametrize("N,steps", [(1, 400), (1024, 90)])
def test_one_step_parity_config_sizes(torch_mod, oracle_mod, N, steps):
    """BASELINE configs[0] shape (N = 1) and configs[1] (N = 1024): random-action rollout from reset, GPU resynchronised to the
    oracle before every step; contact sets / done flags equal, pose and force error percentiles as in the N = 32 test."""
    torch = torch_mod
    o = oracle_mod.Oracle(N, omp=N > 64, residual_threshold=0.0, warmstart=0.0, seed=21)
    led = P.ConditionedParity(oracle_mod, with_cache=False, residual_threshold=0.0, warmstart=0.0)
    g = _gpu(N, residual_threshold=0.0, warmstart=0.0, seed=21)
    rng = np.random.default_rng(3)
    perr, ferr, oerr = [], [], []
    maxc = 0
    for t in range(steps):
        a = rng.uniform(-1, 1, (N, 4))
        _to_gpu_state(torch, g, o.get_state()); led.before(o)
        oo, ro, do = o.step(a)
        og, rg, dg = g.step(torch.tensor(a, dtype=torch.float32))
        so = o.get_state(); sg = g.state().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(o.ncontacts(), sg[:, _lib.S_NCONTACT].astype(int))
        np.testing.assert_array_equal(dg.cpu().numpy(), do)
        oerr.append(np.abs(og.cpu().numpy()[:, 2:] - oo[:, 2:]).max(1))                   # ee position
        maxc = max(maxc, int(o.ncontacts().max()))
        perr.append(np.abs(so[:, POS] - sg[:, POS]).max(1))
        cf = o.contact_force(); ferr.append(np.abs(sg[:, _lib.S_CFORCE] - cf) / (1 + np.abs(cf)))
        led.after(o, a, perr[-1], ferr[-1])
    oerr = np.concatenate(oerr)
    res = led.finish("one-step resynchronised N=%d" % N)
    print("N=%d: max contacts %d; obs (ee position) err max %.2e within WELL / %.2e over all env-steps" % (N, maxc, oerr[~res["exempt"]].max(), oerr.max()))
    assert maxc >= 8
    assert oerr[~res["exempt"]].max() < 1e-4 and oerr.max() < 1e-2   # observation (ee position); north_star 1e-3 (the arm is 1e4 x heavier than what makes a step ill-conditioned)


def test_spill_path_many_contacts(torch_mod, oracle_mod):
    """Contacts 21..48 take the global-scratch path of the HIP PGS (second `block` instantiation, sign words sg1 / sg2).
    Pipes coiled flat on the table (25 table + up to ~17 self contacts) in scripted mode, so that the gripper later comes
    down on the coil and closes (finger / arm contacts at slots >= 25): GPU resynchronised to the oracle before every checked
    step; contact count, contact keys, link pairs, points / normals, per-contact normal impulse, pose and contact force are
    compared and the counts the test reached are ASSERTED (> 20 and > 32).  Every env-step is bounded (tests/parity_util.py): within
    1e-4, or -- the gripper closing with 20 kN on a mu = 10 link -- within 10 x the fp64 oracle's own spread under 1e-6 perturbations;
    the share of the latter is asserted (< 10 %)."""
    torch = torch_mod
    from tests.scenarios import coil_pipe_flat
    N = 8
    kw = dict(mode=1, dv=0.05, residual_threshold=0.0, warmstart=0.0)
    o = oracle_mod.Oracle(N, **kw); g = _gpu(N, debug=1, **kw); led = P.ConditionedParity(oracle_mod, with_cache=False, slots=128, **kw)
    o.set_state(coil_pipe_flat(o.get_state()))
    a = np.zeros((N, 4)); at = torch.zeros(N, 4)
    perr, ferr, lerr = [], [], []
    seen = np.zeros(49, int); arm_spilled = 0
    for t in range(1150):
        check = t < 40 or 600 <= t < 760 or 1015 <= t < 1150
        if check:
            _to_gpu_state(torch, g, o.get_state()); led.before(o)
        o.step(a)
        if not check:
            continue
        g.step(at)
        so = o.get_state(); sg = g.state().cpu().numpy().astype(np.float64)
        nco = o.ncontacts()
        np.testing.assert_array_equal(nco, sg[:, _lib.S_NCONTACT].astype(int))
        dbg = g.debug().cpu().numpy().astype(np.float64)
        for e in range(N):
            oc = o.debug_contacts(e); k = len(oc)
            gc = dbg[e, _lib.DBG_CONTACT:_lib.DBG_CONTACT + _lib.DBG_CONTACT_STRIDE * k].reshape(k, _lib.DBG_CONTACT_STRIDE)
            np.testing.assert_array_equal(oc[:, 10], gc[:, _lib.DBG_CONTACT_KEY])                      # same contact keys, same order
            np.testing.assert_array_equal(oc[:, 0:2], gc[:, 0:2])                    # same link pairs
            np.testing.assert_allclose(oc[:, 2:9], gc[:, 2:9], atol=1e-4)            # point, normal, depth (fp32 kinematics of a 1.3 m chain)
            seen[k] += 1
            arm_spilled += int(((oc[20:, 0] < 9) | ((oc[20:, 1] >= 0) & (oc[20:, 1] < 9))).sum())
            lerr.append(np.abs(oc[:, 11] - gc[:, _lib.DBG_CONTACT_LAMBDA]).max() / (1e-3 + np.abs(oc[:, 11]).max()) if k else 0.0)
        perr.append(np.abs(so[:, POS] - sg[:, POS]).max(1))
        cf = o.contact_force(); ferr.append(np.abs(sg[:, _lib.S_CFORCE] - cf) / (1 + np.abs(cf)))
        led.after(o, a, perr[-1], ferr[-1])
    res = led.finish("spill path (21..48 contacts)", exempt_share=0.10, p99=1e-4)
    lerr = np.array(lerr); ok = ~res["exempt"]
    print("spill path: max contacts %d, with > 20 contacts %d, with > 32 contacts %d, arm-involving contacts in spilled slots %d" % (
        seen.nonzero()[0].max(), seen[21:].sum(), seen[33:].sum(), arm_spilled))
    print("spill path: lambda_n rel err well-conditioned p50/p99/max = %.2e / %.2e / %.2e" % (np.percentile(lerr[ok], 50), np.percentile(lerr[ok], 99), lerr[ok].max()))
    assert seen[21:].sum() > 300 and seen[33:].sum() > 80 and arm_spilled > 50
    assert np.percentile(lerr[ok], 50) < 2e-3 and np.percentile(lerr[ok], 99) < 5e-2


def test_row_space_and_dof_space_pgs_agree(torch_mod, oracle_mod):
    """Envs with <= 10 contacts are solved in row space with one row per lane (pgs_rows), 11..32 contacts with two rows per lane and
    streamed matrix columns (pgs_rows2), the rest in DOF space; solver_path = 1 forces DOF space for every env.  Same row sequence, so
    from identical states the two must agree to fp32 rounding; and both against the oracle.  The shares of env-steps that took each
    row-space form are asserted (state word 114 = which solver ran), and the two-rows-per-lane steps are bounded on their own."""
    torch = torch_mod
    N = 256
    kw = dict(residual_threshold=0.0, seed=4)
    o = oracle_mod.Oracle(N, omp=True, warmstart=0.85, **kw)
    led_o = P.ConditionedParity(oracle_mod, warmstart=0.85, **kw); led_b = P.ConditionedParity(oracle_mod, warmstart=0.85, **kw)
    ga = _gpu(N, solver_path=0, **kw); gb = _gpu(N, solver_path=1, **kw)
    rng = np.random.default_rng(1)
    dab, dao, lamd, fast, two, dab2, dao2 = [], [], [], 0, 0, [], []
    for t in range(160):
        a = rng.uniform(-1, 1, (N, 4))
        s = o.get_state(); led_o.before(o); led_b.before(o)
        if t > 0:       # physical state AND warm-start cache from the oracle (after an ill-conditioned step the three caches are far apart)
            wc = o.warm_cache()
            for g in (ga, gb):
                st = g.state().cpu().numpy().astype(np.float64); st[:, :_lib.S_TIP] = s[:, :_lib.S_TIP]; st[:, _lib.S_CACHE_N : _lib.S_CACHE_LAMBDA + 48] = wc; g.set_state(torch.tensor(st, dtype=torch.float32))
        o.step(a); ta = torch.tensor(a, dtype=torch.float32)
        ga.step(ta); gb.step(ta)
        sa = ga.state().cpu().numpy().astype(np.float64); sb = gb.state().cpu().numpy().astype(np.float64); so = o.get_state()
        np.testing.assert_array_equal(sa[:, _lib.S_NCONTACT], sb[:, _lib.S_NCONTACT])
        fast += int((sa[:, _lib.S_NCONTACT] <= 10).sum())
        assert (sb[:, _lib.S_SOLVER] == 0).all() and (sa[:, _lib.S_SOLVER][sa[:, _lib.S_NCONTACT] <= 10] != 5).all() and (sa[:, _lib.S_SOLVER][sa[:, _lib.S_NCONTACT] <= 10] != 0).all()
        m2 = sa[:, _lib.S_SOLVER] == 5
        assert np.array_equal(m2, (sa[:, _lib.S_NCONTACT] > 10) & (sa[:, _lib.S_NCONTACT] <= 32))
        two += int(m2.sum())
        dab.append(np.abs(sa[:, POS] - sb[:, POS]).max(1)); dao.append(np.abs(sa[:, POS] - so[:, POS]).max(1))
        led_o.after(o, a, dao[-1]); led_b.after(o, a, dab[-1])
        dab2.append(dab[-1][m2]); dao2.append(dao[-1][m2])
        lamd.append(np.abs(sa[:, _lib.S_CACHE_LAMBDA : _lib.S_CACHE_LAMBDA + 48] - sb[:, _lib.S_CACHE_LAMBDA : _lib.S_CACHE_LAMBDA + 48]).max(1))      # cached normal impulses
    dab = np.concatenate(dab); dao = np.concatenate(dao); lamd = np.concatenate(lamd)
    assert np.percentile(lamd, 99) < 2e-4 and (lamd > 5e-3).mean() < 2e-3        # rare ill-conditioned steps (tests/scenarios.py)
    print("row-space vs DOF-space PGS: %d of %d env-steps in row space; pose diff p50/p99/max %.2e / %.2e / %.2e ; vs oracle p50/p99 %.2e / %.2e" % (
        fast, N * 160, np.percentile(dab, 50), np.percentile(dab, 99), dab.max(), np.percentile(dao, 50), np.percentile(dao, 99)))
    assert fast > 0.5 * N * 160
    dab2 = np.concatenate(dab2); dao2 = np.concatenate(dao2)
    print("   two rows per lane: %d env-steps; pose diff vs DOF space p50/p99 %.2e / %.2e ; vs oracle p50/p99 %.2e / %.2e" % (
        two, np.percentile(dab2, 50), np.percentile(dab2, 99), np.percentile(dao2, 50), np.percentile(dao2, 99)))
    assert two > 300
    assert np.percentile(dab2, 50) < 5e-6 and np.percentile(dab2, 90) < 2e-4
    assert np.percentile(dab, 50) < 2e-6 and np.percentile(dab, 99) < 2e-4
    # and on EVERY env-step
    led_o.finish("row space vs oracle", p99=5e-5, check_force=False)
    led_b.finish("row space vs DOF space", p99=5e-5, p50=2e-6, check_force=False)


@pytest.mark.parametrize("bent", [False, True])
def test_trajectory_parity_contact_stable(torch_mod, oracle_mod, bent):
    """1000 steps, identical seeds: peg-tip pose <= 1e-3 m, contact-normal force <= 1e-2 N, obs <= 1e-3."""
    torch = torch_mod
    N = 8
    kw = dict(residual_threshold=0.0)
    o = oracle_mod.Oracle(N, **kw); g = _gpu(N, **kw)
    p0, _ = oracle_mod.fk_arm(REST, 9)
    if bent:
        a = np.tile([p0[0], p0[1], p0[2], 0.0], (N, 1))
        for _ in range(1000):
            o.step(a)
        s = o.get_state(); s[:, _lib.S_VLIN : _lib.S_QJ] = 0; s[:, _lib.S_QDJ : _lib.S_TARGET] = 0; o.set_state(s)
    else:
        s = o.get_state(); s[:, _lib.S_QJ : _lib.S_QDJ] = 0; s[:, _lib.S_POS + 2] = -0.04 + 1e-4; o.set_state(s)
    _to_gpu_state(torch, g, s)
    maxd = maxo = 0.0
    led = P.ForceLedger(oracle_mod, slots=128, **kw)
    for t in range(1000):
        ph = 2 * np.pi * t / 500.0
        a = np.tile([p0[0] + 0.1 * np.sin(ph), p0[1] + 0.1 * np.cos(ph) - 0.1, p0[2] + 0.05 * np.sin(2 * ph), 0.02], (N, 1))
        led.before(o)
        oo, _, _ = o.step(a)
        og, _, _ = g.step(torch.tensor(a, dtype=torch.float32))
        maxd = max(maxd, np.abs(o.tip_pose()[:, :3] - g.tip_pose().cpu().numpy()[:, :3]).max())
        maxo = max(maxo, np.abs(oo - og.cpu().numpy()).max())
        led.after(a, o.contact_force(), g.contact_force().cpu().numpy())
    print("trajectory parity bent=%s: tip %.3e m, obs %.3e" % (bent, maxd, maxo))
    # north_star's 1e-2 N on every step whose force the oracle's own probes find stable, 16-step mean everywhere; transients classified
    # by probes and bounded by 10 x the probes' deviation (tests/parity_util.py ForceLedger)
    led.finish("trajectory parity (exit test off) bent=%s" % bent)
    assert maxd < 1e-3 and maxo < 1e-3, (maxd, maxo)


def test_gpu_matches_host_emulation_of_same_source(torch_mod):
    """The fp32 host build of the same device source must agree with the GPU to fp32 rounding over a short chaotic
    rollout: catches wave-primitive / LDS-synchronisation bugs that an algorithmic oracle cannot localise."""
    torch = torch_mod
    from tests.emul import emul as E
    E.build()
    N = 16
    g = _gpu(N, residual_threshold=0.0); e = E.Emul(N, "f32", residual_threshold=0.0)
    rng = np.random.default_rng(5)
    for t in range(40):
        a = rng.uniform(-1, 1, (N, 4)).astype(np.float32)
        se = e.get_state(); g.set_state(torch.tensor(se, dtype=torch.float32))
        e.step(a.astype(np.float64)); g.step(torch.tensor(a))
        sg = g.state().cpu().numpy().astype(np.float64); se = e.get_state()
        assert np.abs(sg[:, POS] - se[:, POS]).max() < 5e-4
        np.testing.assert_array_equal(sg[:, _lib.S_NCONTACT], se[:, _lib.S_NCONTACT])


def test_spill_path_matches_host_emulation(torch_mod):
    """The same > 20 / > 32 contact scenario against the fp32 HOST build of the same algorithm (tests/emul): isolates what is
    specific to the gfx950 wave layer (global-scratch records, sign words sg1 / sg2, lane-32 store visibility) from fp32
    sensitivity of the algorithm itself."""
    torch = torch_mod
    from tests.emul import emul as E
    from tests.scenarios import coil_pipe_flat
    E.build()
    N = 8
    kw = dict(mode=1, dv=0.05, residual_threshold=0.0, warmstart=0.0)
    g = _gpu(N, **kw); e = E.Emul(N, "f32", **kw)
    se = e.get_state(); se[:, :_lib.S_TIP] = coil_pipe_flat(se[:, :_lib.S_TIP].copy()); se[:, _lib.S_CACHE_N] = 0; e.set_state(se)
    at = torch.zeros(N, 4); a = np.zeros((N, 4))
    err, cnt = [], []
    for t in range(1150):
        check = t < 40 or 600 <= t < 760 or 1015 <= t < 1150
        if check:
            st = e.get_state(); st[:, _lib.S_CACHE_N] = 0; e.set_state(st); g.set_state(torch.tensor(st, dtype=torch.float32))
        e.step(a)
        if not check:
            continue
        g.step(at)
        sg = g.state().cpu().numpy().astype(np.float64); se = e.get_state()
        np.testing.assert_array_equal(sg[:, _lib.S_NCONTACT], se[:, _lib.S_NCONTACT])
        err.append(np.abs(sg[:, POS] - se[:, POS]).max(1)); cnt.append(se[:, _lib.S_NCONTACT].copy())
    err = np.concatenate(err); cnt = np.concatenate(cnt)
    for lo, hi in ((0, 10), (11, 20), (21, 32), (33, 48)):
        m = (cnt >= lo) & (cnt <= hi)
        if m.any():
            print("GPU vs fp32 host build, %2d..%2d contacts: %4d env-steps, pose diff p50 %.2e p99 %.2e max %.2e" % (lo, hi, m.sum(), np.percentile(err[m], 50), np.percentile(err[m], 99), err[m].max()))
    assert (cnt > 20).sum() > 300 and (cnt > 32).sum() > 100
    # medians at rounding level in every bracket; the tail is the ill-conditioned steps with the gripper pressing on a mu = 10 link
    # (two fp32 builds of one algorithm amplify their rounding differences there, tests/scenarios.py), absent in the static > 32 bracket
    assert np.percentile(err, 50) < 2e-6 and np.percentile(err, 90) < 5e-5 and err[cnt > 32].max() < 5e-4


def test_free_fall_and_resting_force_on_gpu(torch_mod, oracle_mod):
    torch = torch_mod
    g = _gpu(4, enable_self_collision=0)
    st = g.state().cpu().numpy(); st[:, _lib.S_POS + 2] = 1.0; g.set_state(torch.tensor(st))
    p0, _ = oracle_mod.fk_arm(REST, 9)
    a = torch.tensor(np.tile([p0[0], p0[1], p0[2], 0.0], (4, 1)), dtype=torch.float32)
    z, v, dt = 1.0, 0.0, 1 / 240
    for n in range(40):
        g.step(a)
        v += dt * (-9.8 - 0.04 * v * (1 + abs(v))); z += dt * v
    st = g.state().cpu().numpy()
    np.testing.assert_allclose(st[:, _lib.S_POS + 2], z, atol=2e-5); np.testing.assert_allclose(st[:, _lib.S_VLIN + 2], v, atol=2e-4)
    g2 = _gpu(4)
    for _ in range(1500):
        g2.step(a)
    f = torch.stack([(g2.step(a), g2.contact_force())[1] for _ in range(60)]).mean(0).cpu().numpy()
    np.testing.assert_allclose(f, 2.6215, atol=1e-2)       # m g of the 25-link pipe


def test_full_size_properties(torch_mod):
    """BASELINE config sizes (4096 envs, random actions): finite state, unit quaternions, joint limits respected,
    bitwise run-to-run determinism, auto-reset keeps every env alive, done/reward consistent."""
    torch = torch_mod
    N = 4096
    outs = []
    for rep in range(2):
        g = _gpu(N, auto_reset=1, max_episode_steps=64, seed=11)
        gen = torch.Generator(device="cuda").manual_seed(1234)
        for t in range(100):
            a = torch.rand(N, 4, device="cuda", generator=gen) * 2 - 1
            obs, rew, done = g.step(a)
        torch.cuda.synchronize()
        st = g.state()
        outs.append(st.clone())
        assert torch.isfinite(st).all()
        q = st[:, _lib.S_QUAT : _lib.S_VLIN]
        assert torch.allclose(q.norm(dim=1), torch.ones(N, device="cuda"), atol=1e-4)
        lo = torch.tensor([-2.9671, -1.8326, -2.9671, -3.1416, -2.9671, -0.0873, -2.9671, 0.0, 0.0], device="cuda")
        hi = torch.tensor([2.9671, 1.8326, 2.9671, 0.0, 2.9671, 3.8223, 2.9671, 0.04, 0.04], device="cuda")
        assert (st[:, _lib.S_QARM : _lib.S_QDARM] >= lo - 0.05).all() and (st[:, _lib.S_QARM : _lib.S_QDARM] <= hi + 0.05).all()
        steps = st[:, _lib.S_STEPS]
        assert (steps >= 0).all() and (steps < 64).all()
        assert (steps == 100 % 64).float().mean() > 0.97    # nearly every env auto-reset once, in lockstep (a few finish early: reward)
        assert st[:, _lib.S_SPARE].sum().item() == 0                   # no env was ever reset because of a non-finite state
        assert (st[:, _lib.S_POS + 2] > -0.2).all()                 # nothing tunnelled through the table
    assert torch.equal(outs[0], outs[1])


def test_scripted_mode_on_gpu(torch_mod, oracle_mod):
    """Scripted episodes (reference step() semantics) on the GPU: exact FSM clock, done after 2226 env-steps, and
    resynchronised one-step parity with the oracle through approach / descent / finger closing."""
    torch = torch_mod
    N = 8
    kw = dict(mode=1, dv=0.05, residual_threshold=0.0, warmstart=0.0)
    g = _gpu(N, **kw)
    g.step_n(2225)
    torch.cuda.synchronize()
    st = g.state().cpu().numpy()
    assert (st[:, _lib.S_FSM] == 8).all() and not g.done.cpu().numpy().any()
    g.step_n(1)
    st = g.state().cpu().numpy()
    assert (st[:, _lib.S_FSM] == 9).all() and (st[:, _lib.S_STEPS] == 2226).all() and g.done.cpu().numpy().all()
    assert np.isfinite(st).all()

    o = oracle_mod.Oracle(N, **kw); led = P.ConditionedParity(oracle_mod, with_cache=False, slots=128, **kw)
    g2 = _gpu(N, **kw)
    a = np.zeros((N, 4)); at = torch.zeros(N, 4)
    for t in range(1350):
        check = t < 100 or 560 <= t < 660 or 1020 <= t < 1150 or 1262 <= t < 1350      # last window: attach constraint active
        if check:
            _to_gpu_state(torch, g2, o.get_state()); led.before(o)
        o.step(a)
        if check:
            g2.step(at)
            so = o.get_state(); sg = g2.state().cpu().numpy().astype(np.float64)
            np.testing.assert_array_equal(so[:, _lib.S_FSM], sg[:, _lib.S_FSM])
            np.testing.assert_array_equal(o.ncontacts(), sg[:, _lib.S_NCONTACT].astype(int))
            np.testing.assert_allclose(so[:, _lib.S_TARGET : _lib.S_FSM], sg[:, _lib.S_TARGET : _lib.S_FSM], atol=2e-4)
            led.after(o, a, np.abs(so[:, POS] - sg[:, POS]).max(1))
    led.finish("scripted one-step (approach / descent / grasp / attach)", exempt_share=0.10, check_force=False)


def test_arm_table_contact_on_gpu(torch_mod, oracle_mod):
    """Arm collision spheres vs the table (keys 3000+, linkA = arm link, no pipe response): drive the gripper into the table,
    GPU resynchronised to the oracle before every step.  Same contact sets, arm stops at the table, small one-step errors."""
    torch = torch_mod
    N = 8
    kw = dict(residual_threshold=0.0, warmstart=0.0)
    o = oracle_mod.Oracle(N, **kw); g = _gpu(N, **kw); led = P.ConditionedParity(oracle_mod, with_cache=False, slots=128, **kw)
    p0, _ = oracle_mod.fk_arm(REST, 9)
    a = np.tile([p0[0] + 0.25, p0[1] - 0.25, -1.0, 0.04], (N, 1))
    seen = 0; lowest = 1.0; variants = np.zeros(6, int)
    for t in range(420):
        _to_gpu_state(torch, g, o.get_state()); led.before(o)
        o.step(a); g.step(torch.tensor(a, dtype=torch.float32))
        so = o.get_state(); sg = g.state().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(o.ncontacts(), sg[:, _lib.S_NCONTACT].astype(int))
        seen += any(int(k) >= 3000 for k in o.debug_contacts(0)[:, 10])
        led.after(o, a, np.abs(so[:, POS] - sg[:, POS]).max(1))
        lowest = min(lowest, oracle_mod.fk_arm(so[0, _lib.S_QARM : _lib.S_QDARM], 9)[0][2])
        variants += np.bincount(sg[:, _lib.S_SOLVER].astype(int), minlength=6)
    print("arm-table: solver variants (state word 114) histogram:", variants.tolist())
    assert seen > 50 and lowest > -0.05 - 0.004
    led.finish("arm-table contacts", exempt_share=0.05, p99=5e-5, check_force=False)


def test_clamped_arm_motor_reruns_with_limit_rows(torch_mod, oracle_mod):
    """The solve that leaves out the limit rows of arm joints 0..6 (pih_wave.h: skip7) is only valid while no arm motor row clamps; the
    multipliers are watched every iteration and a clamp re-runs the solve with every limit row in place (state word 114 = 4).  With the
    action-mode impulse bound of 1e5 dt that does not happen in any other test (416 N s at dt = 1/240); here dt = 1e-3 (bound 100 N s)
    and the arm joints are thrown at up to 400 rad/s every 8th step, which the motors cannot brake within their bound.  One-step
    parity, resynchronised, must hold on that path too."""
    torch = torch_mod
    N = 64
    kw = dict(dt=1e-3, residual_threshold=0.0)
    o = oracle_mod.Oracle(N, seed=3, **kw); g = P.GpuProduct(N, seed=3, **kw); led = P.ConditionedParity(oracle_mod, slots=256, **kw)
    rng = np.random.default_rng(0)
    variants = np.zeros(6, int)
    for t in range(96):
        if t % 8 == 0:
            a = np.c_[rng.uniform(-0.6, 0.6, N), rng.uniform(-0.8, -0.2, N), rng.uniform(0.05, 0.5, N), rng.uniform(0, 0.04, N)]
            s = o.get_state(); s[:, _lib.S_QARM : _lib.S_QDARM] = REST; s[:, _lib.S_QDARM : _lib.S_QDARM + 7] = rng.uniform(-400, 400, (N, 7)); o.set_state(s)
        P.sync_product(g, o); led.before(o)
        o.step(a); g.step(a)
        so = o.get_state(); sg = g.get_state()
        np.testing.assert_array_equal(o.ncontacts(), sg[:, _lib.S_NCONTACT].astype(int))
        led.after(o, a, np.abs(so[:, POS] - sg[:, POS]).max(1))
        variants += np.bincount(sg[:, _lib.S_SOLVER].astype(int), minlength=6)
    print("clamped arm motors (dt = 1e-3): solver variants histogram", variants.tolist())
    assert variants[4] > 50, "the re-run after a clamped arm motor row was not exercised: %s" % variants.tolist()
    led.finish("clamped arm motors, re-run with limit rows", exempt_share=0.02, check_force=False)


def test_joint_limit_rows_on_gpu(torch_mod, oracle_mod):
    """Joint-limit rows active (their multipliers live in wave-uniform registers on the GPU): joints thrown at their limits
    at 50 / 30 rad/s in scripted state 0; closed form pen / dt after the first step, resynchronised parity afterwards."""
    torch = torch_mod
    N = 4
    kw = dict(residual_threshold=0.0, warmstart=0.0, enable_self_collision=0, mode=1, dv=0.05)
    o = oracle_mod.Oracle(N, **kw); g = _gpu(N, **kw)
    s = o.get_state()
    s[:, _lib.S_QARM + 2] = 2.9671 - 0.02; s[:, _lib.S_QDARM + 2] = 50.0; s[1::2, _lib.S_QARM + 3] = -0.01; s[1::2, _lib.S_QDARM + 3] = 30.0; s[:, _lib.S_POS] = 5.0
    o.set_state(s)
    perr = []
    for t in range(20):
        so = o.get_state(); _to_gpu_state(torch, g, so)
        o.step(np.zeros((N, 4))); g.step(torch.zeros(N, 4))
        so = o.get_state(); sg = g.state().cpu().numpy().astype(np.float64)
        perr.append(np.abs(so[:, POS] - sg[:, POS]).max())
        if t == 0:
            assert abs(sg[0, _lib.S_QDARM + 2] - 4.8) < 2e-3 and abs(sg[1, _lib.S_QDARM + 3] - 2.4) < 2e-3
    print("limit-row one-step pose err max = %.2e" % max(perr))
    assert max(perr) < 2e-5 and abs(sg[0, _lib.S_QARM + 2] - 2.9671) < 1e-4 and abs(sg[1, _lib.S_QARM + 3]) < 1e-4


def test_tube_contacts_on_gpu(torch_mod, oracle_mod):
    """Hole-tube contacts (signed distance to the annular tube) are rare in random rollouts: a straight pipe threaded through
    the bore and dropped onto its inner wall, GPU resynchronised to the oracle before every step."""
    torch = torch_mod
    N = 4
    hole = np.array([0.5, -0.2, 0.2]); rin, r = 0.01536, 0.01
    kw = dict(residual_threshold=0.0, warmstart=0.0, enable_self_collision=0)
    o = oracle_mod.Oracle(N, **kw); g = _gpu(N, **kw); led = P.ConditionedParity(oracle_mod, with_cache=False, slots=64, **kw)
    s = o.get_state()
    s[:, _lib.S_QJ : _lib.S_QDJ] = 0
    s[:, _lib.S_POS] = hole[0] - np.array([0.30, 0.45, 0.60, 0.75]); s[:, _lib.S_POS + 1] = hole[1]; s[:, _lib.S_POS + 2] = hole[2] - (rin - r - 0.002)
    s[:, _lib.S_QUAT : _lib.S_VLIN] = [0, 0, np.sin(-np.pi / 4), np.cos(-np.pi / 4)]; s[:, _lib.S_VLIN : _lib.S_QJ] = 0
    o.set_state(s)
    a = np.tile([0.3, 0.0, 0.5, 0.0], (N, 1))
    ntube = 0
    for t in range(60):
        so = o.get_state(); _to_gpu_state(torch, g, so); led.before(o)
        o.step(a); g.step(torch.tensor(a, dtype=torch.float32))
        so = o.get_state(); sg = g.state().cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(o.ncontacts(), sg[:, _lib.S_NCONTACT].astype(int))
        ntube += sum(100 <= int(k) < 300 for k in o.debug_contacts(0)[:, 10])
        led.after(o, a, np.abs(so[:, POS] - sg[:, POS]).max(1))
    assert ntube > 100
    led.finish("tube contacts", exempt_share=0.05, p99=5e-5, check_force=False)
