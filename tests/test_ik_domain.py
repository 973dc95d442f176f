"""calculateInverseKinematics (envs/utils.py:67,79) over its whole input domain, on the CPU: the case classes of tests/ik_cases.py
(A arithmetic, B fixed point, C exit test in mid-loop, D sign symmetry of the target quaternion) for the Panda and the UR5 chain.

  * the oracle's DLS step is pinned by a plain numpy restatement (one iteration; Jacobians from the oracle, which are checked against
    finite differences elsewhere): a sign error of the orientation term would not show at zero orientation error;
  * the host builds of the product source (tests/emul: serial ik_chain of pih_common.h, and ikq_solve of pih_ikq.h with the four lanes
    of a quad as four threads in lockstep) against the oracle: fp64 within 1e-8, fp32 within 2 x the maxima recorded below, so that a
    change of the arithmetic shows;
  * sincos_joint<float> (pih_math.h) against fp64 sin / cos on a dense grid and around every multiple of pi/4.

The GPU build of the same source is held to 8 x the same recorded maxima (tests/test_gpu_ik.py)."""
import numpy as np
import pytest

from tests import ik_cases as K
from tests.emul import emul as E

# max |q* - oracle| of the fp32 host builds (the larger of serial and quad), measured with the seeds of tests/ik_cases.py
F32_HOST_MAX_A = {
    "ur5": {(0.5, 20): 4.809e-06, (0.5, 1): 9.910e-07, (0.5, 50): 5.881e-06, (0.05, 1): 2.230e-06, (0.05, 3): 5.326e-06},
    "panda": {(0.5, 20): 3.397e-06, (0.5, 1): 5.155e-07, (0.5, 50): 2.306e-06, (0.05, 1): 1.601e-06, (0.05, 3): 4.884e-06},
}
F32_HOST_MAX_C = {"ur5": 4.135e-06, "panda": 7.202e-07}     # class C, the cases that are not threshold-sensitive (a sensitive case: 2 x the oracle's own band)
F32_HOST_MAX_D = {"ur5": 6.676e-06, "panda": 4.031e-06}     # class D: max |q*(tquat) - q*(-tquat)|
F64_TOL = 1e-8
MAXSTEP = 30.0 * np.pi / 180.0


@pytest.fixture(scope="module", autouse=True)
def _build(oracle_mod):
    E.build()


def host(chain, kind, prec, case, damping=K.DEFAULT[0], iters=K.DEFAULT[1], residual=K.RESIDUAL):
    """q* [n, WORDS] of a host build: kind 'serial' = ik_chain, 'quad' = ikq_solve"""
    cfg = E.default_config(prec, ik_damping=damping, ik_iters=iters, ik_residual=residual)
    q0, tp, tq = case["q0"], case["tpos"], case["tquat"]
    if kind == "serial":
        f = E.ik_ur5 if chain == "ur5" else E.ik
        return np.array([f(q0[i], tp[i], tq[i], prec, cfg) for i in range(len(q0))])
    return np.array([E.ikq(q0[i], tp[i], tq[i], prec, cfg, ur5=chain == "ur5")[0] for i in range(len(q0))])


KINDS = ("serial", "quad")


# ------------------------------------------------------------------------------------------------ the oracle's DLS step, in numpy
def _dls_step(O, chain, q0, tpos, tquat, damping):
    n = K.ARM[chain]
    p, qe = K.fk(O, chain, q0)
    Jl, Ja = O.jacobian_ur5(q0) if chain == "ur5" else O.jacobian_ee(q0)
    J = np.vstack([Jl[:, :n], Ja[:, :n]])
    d = K.q_mul(tquat, np.array([-qe[0], -qe[1], -qe[2], qe[3]]))
    sn = np.linalg.norm(d[:3])
    ang = 2 * np.arctan2(sn, d[3])
    if ang > np.pi:
        ang -= 2 * np.pi
    e = np.concatenate([tpos - p, ang * d[:3] / sn])
    dq = J.T @ np.linalg.solve(J @ J.T + damping * np.eye(6), e)
    mx = np.abs(dq).max()
    out = q0.copy()
    out[:n] += dq * (MAXSTEP / mx if mx > MAXSTEP else 1.0)
    return out, mx > MAXSTEP


def test_oracle_dls_step_pinned_by_numpy(oracle_mod):
    """one iteration of the oracle = q0 + J^T (J J^T + d I)^-1 [tpos - p ; angle * axis of tq * conj(q_ee)], |dq|_inf clamped to 30 degrees"""
    err = 0.0; clamped = 0; total = 0
    for chain in K.CHAINS:
        A = K.class_a(chain)
        for damping in (0.5, 0.05):
            ref = K.ref_a(chain, (damping, 1))
            for i in range(K.N_A):
                out, cl = _dls_step(oracle_mod, chain, A["q0"][i], A["tpos"][i], A["tquat"][i], float(np.float32(damping)))
                err = max(err, np.abs(out - ref[i]).max()); clamped += int(cl); total += 1
    print("   numpy DLS step vs oracle: max %.2e over %d cases, clamp active in %d" % (err, total, clamped))
    assert err < 1e-8
    assert clamped > total // 2


def test_oracle_is_symmetric_in_the_sign_of_the_target_quaternion(oracle_mod):
    for chain in K.CHAINS:
        D = K.class_d(chain)
        r = K.ref_batch(oracle_mod, chain, D["q0"], D["tpos"], D["tquat"], residual=0.0)
        assert np.abs(r[:K.N_A] - r[K.N_A:]).max() < 1e-9
        np.testing.assert_array_equal(r[:K.N_A], K.ref_a(chain))


# ------------------------------------------------------------------------------------------------ host builds of the product source
@pytest.mark.parametrize("cfg", K.CONFIGS_A, ids=lambda c: "d%g-it%d" % c)
@pytest.mark.parametrize("chain", K.CHAINS)
def test_class_a_arithmetic(chain, cfg):
    A = K.class_a(chain); ref = K.ref_a(chain, cfg)
    assert np.abs(ref - A["q0"]).max() > (0.5 if cfg[1] == 1 else 1.5)          # the clamp and several quadrants are exercised
    worst = 0.0
    for kind in KINDS:
        e64 = np.abs(host(chain, kind, "f64", A, cfg[0], cfg[1], 0.0) - ref).max(1)
        e32 = np.abs(host(chain, kind, "f32", A, cfg[0], cfg[1], 0.0) - ref).max(1)
        print("   class A %s %s %s: fp64 max %.2e, fp32 max %.3e p99 %.2e, fp32 by displacement scale %s" % (
            chain, cfg, kind, e64.max(), e32.max(), np.percentile(e32, 99), ["%.2e" % e32[A["scale"] == s].max() for s in K.SCALES]))
        assert e64.max() < F64_TOL
        worst = max(worst, e32.max())
    assert worst <= 2 * F32_HOST_MAX_A[chain][cfg]


@pytest.mark.parametrize("chain", K.CHAINS)
def test_class_b_fixed_point_is_bit_exact(chain):
    B = K.class_b(chain)
    for kind in KINDS:
        for prec in ("f64", "f32"):
            np.testing.assert_array_equal(host(chain, kind, prec, B), B["q0"])


@pytest.mark.parametrize("chain", K.CHAINS)
def test_class_c_exit_test_in_mid_loop(chain):
    Cc = K.class_c(chain); sens = Cc["band"] > 0
    print("   class C %s: %.0f %% exit in mid-loop, %.0f %% threshold-sensitive" % (chain, 100 * Cc["exits"].mean(), 100 * sens.mean()))
    worst = 0.0
    for kind in KINDS:
        e64 = np.abs(host(chain, kind, "f64", Cc) - Cc["ref"]).max(1)
        e32 = np.abs(host(chain, kind, "f32", Cc) - Cc["ref"]).max(1)
        print("   class C %s %s: fp64 max %.2e, fp32 max not sensitive %.3e, sensitive %.2e (largest share of its bound %.2f)" % (
            chain, kind, e64.max(), e32[~sens].max(), e32[sens].max(), (e32 / K.class_c_bound(Cc, 2 * F32_HOST_MAX_C[chain])).max()))
        assert (e64 <= K.class_c_bound(Cc, F64_TOL)).all()
        assert (e32 <= K.class_c_bound(Cc, 2 * F32_HOST_MAX_C[chain])).all()
        worst = max(worst, e32[~sens].max())
    assert worst <= 2 * F32_HOST_MAX_C[chain]


@pytest.mark.parametrize("chain", K.CHAINS)
def test_class_d_sign_symmetry(chain):
    D = K.class_d(chain)
    worst = 0.0
    for kind in KINDS:
        o64 = host(chain, kind, "f64", D, residual=0.0); o32 = host(chain, kind, "f32", D, residual=0.0)
        d64 = np.abs(o64[:K.N_A] - o64[K.N_A:]).max(); d32 = np.abs(o32[:K.N_A] - o32[K.N_A:]).max()
        print("   class D %s %s: |q*(tq) - q*(-tq)| fp64 %.2e, fp32 %.3e" % (chain, kind, d64, d32))
        assert d64 < F64_TOL
        worst = max(worst, d32)
    assert worst <= 2 * F32_HOST_MAX_D[chain]


# ------------------------------------------------------------------------------------------------ sincos_joint<float>
def test_sincos_joint_f32_error_bound():
    """|error| < 1.2e-7 against fp64 sin / cos of the same fp32 argument (the figure in pih_math.h; measured 9.2e-8), over
    |a| <= 64 -- beyond the 'few tens of radians' a joint angle reaches in the IK loop -- and at the quadrant boundaries of the reduction"""
    grid = np.linspace(-64, 64, 1_200_001).astype(np.float32)
    k = np.arange(-81, 82) * (np.pi / 4)                                   # every multiple of pi/4 within +-64, and its 4 fp32 neighbours on each side
    near = [k.astype(np.float32)]
    for direction in (-np.inf, np.inf):
        x = k.astype(np.float32)
        for _ in range(4):
            x = np.nextafter(x, np.float32(direction)); near.append(x)
    a = np.concatenate([grid] + near)
    s, c = E.sincos_joint(a)
    a64 = a.astype(np.float64)
    es = np.abs(s.astype(np.float64) - np.sin(a64)).max(); ec = np.abs(c.astype(np.float64) - np.cos(a64)).max()
    print("   sincos_joint<float>: max |sin error| %.2e, max |cos error| %.2e over %d arguments" % (es, ec, a.size))
    assert es < 1.2e-7 and ec < 1.2e-7
    quad = np.rint(a64 * (2 / np.pi)).astype(int) & 3
    assert np.bincount(quad, minlength=4).min() > 250_000                      # every quadrant of the Cody-Waite reduction
