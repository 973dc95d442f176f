"""Shared helpers of the HIP-vs-oracle parity tests (test infrastructure).

CONDITIONING -- how the parity tests bound EVERY env-step, not percentiles.  On the overwhelming majority of env-steps one dt of
the (fp64) oracle moves by ~1e-7 when its input is perturbed by 1e-7 (relative); on a few tenths of a percent it moves by
millimetres to tens of centimetres -- a loaded contact of the pipe's 11-gram end links (URDF lateral friction 100, clamped to mu = 10,
pyramid friction) under a fast motion, where 50 Gauss-Seidel sweeps are not a contraction and ANY perturbation (input rounding to the
product's fp32 state record, summation order, fp32 arithmetic) is amplified within the step, chaotically: the response to a
perturbation is heavy-tailed, a clamp or an unloading contact that one perturbation flips multiplies it by another 100.  No
implementation can be held to 1e-3 m there: two fp64 implementations differ by centimetres.  `ConditionedParity` therefore measures,
for every env-step whose product-vs-oracle error exceeds SUSPECT, what the oracle ITSELF does: 2 x K = 32 fp64 probe runs of that
env-step from copies of the input state perturbed by random relative errors of 1e-6 and of 1e-5 (the size of fp32 arithmetic error in
intermediate results and of its accumulation over 50 sweeps); the env-step is ILL-CONDITIONED when any probe deviates from the
unperturbed oracle result by more than AMP = 30 times its perturbation.  This classification never looks at the product.  Asserted:
        well-conditioned env-steps (all but a few tenths of a percent):   error <= NORTH = 1e-3 m / rad, the north_star tolerance, as a MAX
        ill-conditioned env-steps:   error <= max(NORTH, K_SPREAD x the largest deviation any of the oracle's own 32 probes showed on
                                     THAT env-step), K_SPREAD = 10: the licence scales with the measured amplification -- an env-step
                                     that amplifies 30-fold is held to ~3e-3, one that throws the pipe by 0.8 rad to 8.  The product's
                                     error is one more draw from the heavy-tailed response the probes sample, so a FEW env-steps may
                                     exceed 10 x the largest of 32 draws: they are counted and their share of ALL env-steps asserted
                                     <= SPREAD_EXC = 1e-4 (+1 env-step); every error < 1.5 (the state stays sane: no NaN, no blow-up);
                                     the share of ill-conditioned env-steps itself is asserted (`ill_share`, default = exempt_share)
plus the DISTRIBUTION: the share of env-steps above WELL = 1e-4 (default < 1 %), the median and the 99th percentile of the rest.  An
arbitrarily wrong env-step cannot hide: it is either bounded at 1e-3, or it sits on a step where the fp64 oracle amplifies a 1e-6
perturbation more than 30-fold -- those are counted -- and there it is bounded by what the oracle itself does."""
import numpy as np

from peg_in_hole_gym_amd import _lib

POS = [*range(_lib.S_QARM, _lib.S_QDARM), *range(_lib.S_POS, _lib.S_VLIN), *range(_lib.S_QJ, _lib.S_QDJ)]      # position-like words of the state record (arm q, base pose, pipe q)
VEL = [*range(_lib.S_QDARM, _lib.S_POS), *range(_lib.S_VLIN, _lib.S_QJ), *range(_lib.S_QDJ, _lib.S_TARGET)]
CACHE0, CACHE1 = _lib.S_CACHE_N, _lib.S_CACHE_LAMBDA + 48


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


class GpuProduct:
    """numpy-level adapter of the HIP product (PihVecEnv through the C ABI) with the surface of tests/emul's host build:
    get_state() -> float64 [n, 256], set_state(array), step(actions) -> (obs, reward, done) as numpy"""

    def __init__(self, n, **cfg):
        import torch
        from peg_in_hole_gym_amd.vec_env import PihVecEnv
        self.torch = torch
        self.env = PihVecEnv(n, **cfg)
        self.cfg = self.env.cfg
        self.n = n

    def get_state(self):
        return self.env.state().cpu().numpy().astype(np.float64)

    def set_state(self, s):
        self.env.set_state(self.torch.tensor(np.asarray(s), dtype=self.torch.float32))

    def step(self, actions):
        o, r, d = self.env.step(self.torch.tensor(np.asarray(actions), dtype=self.torch.float32))
        return o.cpu().numpy().astype(np.float64), r.cpu().numpy().astype(np.float64), d.cpu().numpy()


def sync_product(g, A, with_cache=True):
    """product := oracle A: the 98 physical state words and (with_cache) the warm-start contact cache (product words 128..224);
    with_cache=False empties the product's cache instead.  `g`: GpuProduct or the host build (tests/emul)"""
    st = g.get_state()
    st[:, :_lib.S_TIP] = A.get_state()[:, :_lib.S_TIP]
    if with_cache:
        st[:, CACHE0:CACHE1] = A.warm_cache()
    else:
        st[:, CACHE0] = 0
    g.set_state(st)


def sync_oracle(B, A, with_cache=True, rounded=False):
    """oracle B := oracle A (optionally through fp32 rounding, i.e. exactly what the product receives)"""
    s = A.get_state(); c = A.warm_cache()
    B.set_state(f32(s) if rounded else s)            # (set_state empties B's cache)
    if with_cache:
        B.set_warm_cache(f32(c) if rounded else c)


class ConditionedParity:
    """Ledger of one resynchronised parity test.  usage per step:
           led.before(A)                       # oracle state (and warm-start cache) the step starts from
           A.step(a); product.step(a)
           led.after(A, a, perr, frel)         # perr [n]: max |position-word error|; frel [n] (optional): |dF| / (1 + |F|)
       and at the end  led.finish(name, ...)   # runs the probes for the suspects and asserts (see the module docstring)."""
    SUSPECT, WELL, NORTH, AMP, K, MAGS = 3e-5, 1e-4, 1e-3, 30.0, 16, (1e-6, 1e-5)
    K_SPREAD, SPREAD_EXC = 10.0, 1e-4
    F_SUSPECT, F_WELL = 1e-3, 1e-2

    def __init__(self, oracle_mod, with_cache=True, slots=512, task="peg-in-hole", **cfg):
        cfg.pop("omp", None); cfg.pop("seed", None)
        self.fly = task == "random-fly"
        if self.fly:      # UR5 + free-flying object: 48-word record, 6-dim action, no warm-start cache
            self.probe = oracle_mod.FlyOracle(slots, omp=True, **cfg)
            self.words, self.adim, self.npert, self.wquat, self.pos = _lib.FLY_STATE_WORDS, _lib.FLY_ACTION_DIM, _lib.F_DONE, _lib.F_OQUAT + 3, [*range(_lib.F_Q, _lib.F_QD), *range(_lib.F_OPOS, _lib.F_OVLIN)]
            with_cache = False
        else:
            self.probe = oracle_mod.Oracle(slots, omp=True, **cfg)      # same solver settings as the oracle under test
            self.words, self.adim, self.npert, self.wquat, self.pos = oracle_mod.STATE_WORDS, _lib.ACTION_DIM, _lib.S_TARGET, _lib.S_QUAT + 3, POS
        self.slots = slots
        self.with_cache = with_cache
        self.perr, self.frel, self.sus = [], [], []
        self.count = 0
        self.rng = np.random.default_rng(12345)

    def before(self, A):
        self.s0 = A.get_state()
        self.c0 = A.warm_cache() if self.with_cache else None

    def after(self, A, actions, perr, frel=None):
        perr = np.asarray(perr); n = len(perr)
        frel = np.zeros(n) if frel is None else np.asarray(frel)
        self.perr.append(perr); self.frel.append(frel)
        idx = np.nonzero((perr > self.SUSPECT) | (frel > self.F_SUSPECT))[0]
        if len(idx):
            sa = A.get_state(); fa = sa[:, _lib.F_CFORCE] if self.fly else A.contact_force(); a = np.asarray(actions, dtype=np.float64)
            for e in idx:
                self.sus.append((self.count + e, self.s0[e].copy(), None if self.c0 is None else self.c0[e].copy(), a[e].copy(), sa[e, self.pos].copy(), float(fa[e])))
        self.count += n

    def _amplification(self):
        """(pose amplification, force amplification, pose spread) of every suspect: max over 2 K perturbed fp64 runs of deviation / perturbation
        magnitude (force: deviation of |dF| / (1 + |F|) per unit perturbation), batched through the probe oracle"""
        m = len(self.sus)
        amp = np.zeros(m); ampf = np.zeros(m); spread = np.zeros(m)
        rows = [(i, k, mag) for i in range(m) for mag in self.MAGS for k in range(self.K)]
        for c0 in range(0, len(rows), self.slots):
            ch = rows[c0:c0 + self.slots]
            st = np.zeros((self.slots, self.words)); st[:, self.wquat] = 1; ac = np.zeros((self.slots, self.adim)); ca = np.zeros((self.slots, 97)); ca[:, 1:49] = -1
            for j, (i, k, mag) in enumerate(ch):
                _, s0, c0_, a, _, _ = self.sus[i]
                s = s0.copy(); s[:self.npert] *= 1 + mag * self.rng.uniform(-1, 1, self.npert)
                st[j] = s; ac[j] = a
                if c0_ is not None:
                    ca[j] = c0_
            self.probe.set_state(st)
            if self.with_cache:
                self.probe.set_warm_cache(ca)
            self.probe.step(ac)
            sr = self.probe.get_state(); fr = sr[:, _lib.F_CFORCE] if self.fly else self.probe.contact_force()
            for j, (i, k, mag) in enumerate(ch):
                _, _, _, _, pos, f = self.sus[i]
                d = np.abs(sr[j, self.pos] - pos).max(); df = abs(fr[j] - f) / (1 + abs(f))
                amp[i] = max(amp[i], d / mag); ampf[i] = max(ampf[i], df / mag); spread[i] = max(spread[i], d)
        return amp, ampf, spread

    def finish(self, name, exempt_share=0.01, p50=5e-6, p99=2e-5, f_p50=1e-3, f_p99=1e-2, check_force=True, ill_share=None):
        perr = np.concatenate(self.perr); frel = np.concatenate(self.frel)
        amp_s, ampf_s, spread_s = self._amplification()
        where = np.array([x[0] for x in self.sus], dtype=int)
        amp = np.zeros(len(perr)); ampf = np.zeros(len(perr)); spread = np.zeros(len(perr))
        if len(where):
            amp[where] = amp_s; ampf[where] = ampf_s; spread[where] = spread_s
        ill = amp > self.AMP                   # (only suspects were probed: an env-step below SUSPECT needs no classification)
        exempt = perr > self.WELL
        big = perr > self.NORTH
        well_max = perr[~ill].max()
        print("%s: %d env-steps; pose err p50/p99 %.2e / %.2e ; max over the WELL-conditioned env-steps %.2e ; %d (%.3f %%) above %.0e, %d (%.3f %%) above the north_star's %.0e, all of "
              "them on the %d (%.3f %%) env-steps where the fp64 oracle amplifies a 1e-6 / 1e-5 perturbation more than %.0f-fold (largest error %.2e; oracle's own spread there %.2e)" % (
                  name, len(perr), np.percentile(perr, 50), np.percentile(perr, 99), well_max, exempt.sum(), 100 * exempt.mean(), self.WELL, big.sum(), 100 * big.mean(), self.NORTH,
                  ill.sum(), 100 * ill.mean(), self.AMP, perr.max(), spread[np.argmax(perr)]))
        worst = np.argmax(np.where(ill, 0.0, perr))
        # the ill-conditioned env-steps: bounded by what the oracle's own probes did THERE
        ill_bound = np.maximum(self.NORTH, self.K_SPREAD * spread)
        exc = ill & (perr > ill_bound)
        ratio = perr[ill] / np.maximum(spread[ill], 1e-300)
        print("   margin on the well-conditioned env-steps: max %.2e vs the bound %.0e (%.1fx); ill-conditioned: error / (oracle's largest probe deviation) p50 %.2f p90 %.2f p99 %.2f max %.1f; "
              "%d env-steps (%.1e of all) above max(%.0e, %.0f x probe deviation), allowed %.0e + 1" % (
                  well_max, self.NORTH, self.NORTH / max(well_max, 1e-300), *(np.percentile(ratio, [50, 90, 99]) if ill.any() else (0, 0, 0)), ratio.max() if ill.any() else 0.0,
                  exc.sum(), exc.mean(), self.NORTH, self.K_SPREAD, self.SPREAD_EXC))
        assert well_max <= self.NORTH, "%s: pose error %.3e on a WELL-conditioned env-step (oracle amplification of a perturbation there: %.1f)" % (name, perr[worst], amp[worst])
        assert exempt.mean() < exempt_share, "%s: %.3f %% of the env-steps exceed %.0e" % (name, 100 * exempt.mean(), self.WELL)
        assert ill.mean() < (exempt_share if ill_share is None else ill_share), "%s: %.3f %% of the env-steps are ill-conditioned" % (name, 100 * ill.mean())
        assert np.percentile(perr, 50) < p50 and np.percentile(perr[~exempt], 99) < p99      # (p99 over the env-steps within WELL)
        assert exc.sum() <= self.SPREAD_EXC * len(perr) + 1, "%s: %d ill-conditioned env-steps exceed %.0f x the oracle's own largest probe deviation (worst: error %.3e, probes %.3e)" % (
            name, exc.sum(), self.K_SPREAD, perr[exc].max(), spread[exc][np.argmax(perr[exc])])
        assert perr.max() < 1.5
        if check_force:
            fill = (ampf > self.AMP) | ill
            fex = frel > self.F_WELL
            print("   contact force |dF| / (1 + |F|): p50/p99 %.2e / %.2e ; max over the well-conditioned env-steps %.2e ; %d (%.3f %%) above %.0e" % (
                np.percentile(frel, 50), np.percentile(frel, 99), frel[~fill].max(), fex.sum(), 100 * fex.mean(), self.F_WELL))
            assert frel[~fill].max() <= self.F_WELL, "%s: force error %.3e (relative) on a well-conditioned env-step" % (name, frel[~fill].max())
            assert fex.mean() < exempt_share and np.percentile(frel, 50) < f_p50 and np.percentile(frel[~fex], 99) < f_p99
        return dict(perr=perr, exempt=exempt, spread=spread, ill=ill, amp=amp)


def defaults_one_step_check(name, oracle_mod, product, N, steps, seed=5, expect_variants=None, omp=True):
    """The check of tests/test_gpu_defaults.py (see its header), on any implementation of the product algorithm: `product` = GpuProduct
    (the HIP library) or tests/emul's host build -- both at the library defaults (residual_threshold 1e-7, warmstart 0.85,
    exit_check_stride 16).  Random-action rollout from reset, product and same-cadence oracle B resynchronised to oracle A (Bullet's
    cadence) before every step."""
    A = oracle_mod.Oracle(N, omp=omp, seed=seed)
    B = oracle_mod.Oracle(N, omp=omp, seed=seed, exit_check_stride=16)
    led = ConditionedParity(oracle_mod, with_cache=True)
    rng = np.random.default_rng(8)
    dA, dB, itA, variants, oerr = [], [], [], [], []
    flips = 0; flip_err = []
    for t in range(steps):
        a = rng.uniform(-1, 1, (N, 4))
        sync_product(product, A); sync_oracle(B, A); led.before(A)
        oo, ro, do = A.step(a); B.step(a)
        og, rg, dg = product.step(a)
        sa = A.get_state(); sg = product.get_state()
        # same contact sets and done flags -- except where a sample sphere sits within float rounding of the contact margin (or the tip of
        # the success radius): such an env-step took another DISCRETE branch than the oracle; counted, its raw pose error recorded and
        # bounded at 1e-2 below, left out of the error statistics of this step
        same = (A.ncontacts() == sg[:, _lib.S_NCONTACT].astype(int)) & (np.asarray(dg).astype(bool) == do.astype(bool))
        flips += int((~same).sum())
        if not same.all():
            flip_err.append(np.abs(sa[~same][:, POS] - sg[~same][:, POS]).max(1))
        cf = A.contact_force()
        led.after(A, a, np.where(same, np.abs(sa[:, POS] - sg[:, POS]).max(1), 0.0), np.where(same, np.abs(sg[:, _lib.S_CFORCE] - cf) / (1 + np.abs(cf)), 0.0))
        oerr.append(np.where(same, np.abs(np.asarray(og)[:, 2:] - oo[:, 2:]).max(1), 0.0))
        gi = sg[:, _lib.S_PGS_ITERS].astype(int)
        dA.append(np.where(same, gi - A.pgs_iters(), 0)); dB.append(np.where(same, gi - B.pgs_iters(), 0)); itA.append(A.pgs_iters().copy()); variants.append(sg[:, _lib.S_SOLVER].astype(int))
    dA, dB, itA, variants, oerr = map(np.concatenate, (dA, dB, itA, variants, oerr))
    res = led.finish(name)
    perr, ok = res["perr"], ~res["exempt"]
    fe = np.concatenate(flip_err) if flip_err else np.zeros(0)
    print("   discrete-branch flips (contact count or done flag differs from the oracle's): %d of %d env-steps, pose error there max %.2e" % (flips, N * steps, fe.max() if len(fe) else 0.0))
    assert flips <= 2e-5 * N * steps + 1
    assert not len(fe) or fe.max() < 1e-2      # a contact at the edge of the margin carries almost no impulse: the flipped step stays close
    print("   early exit (oracle at Bullet's cadence < 50 iterations) in %.1f %% of the env-steps" % (100 * (itA < 50).mean()))
    print("   iterations: product - oracle(Bullet cadence) min/max %d / %d, != 0 in %.2f %% ; product - oracle(product's cadence) != 0 in %.3f %%, max |.| %d" % (
        dA.min(), dA.max(), 100 * (dA != 0).mean(), 100 * (dB != 0).mean(), np.abs(dB).max()))
    print("   obs (ee position) err max %.2e ; solver variants (state word 114) histogram: %s" % (oerr[ok].max(), np.bincount(variants, minlength=6).tolist()))
    # the exit test fired in a meaningful share of the env-steps (free fall / light envs)
    assert (itA < 50).mean() > 0.02
    if expect_variants is not None:
        expect_variants(variants)
    # cadence: the same iteration count as the oracle run at the product's cadence, and at most stride - 1 = 15 further iterations than
    # Bullet's cadence -- except where the residual HOVERS at the threshold (it is not monotone: an env can meet the threshold in
    # iteration 33, miss it in the tested iteration 36 and run to 50; or meet it in fp32 and miss it in fp64).  Those env-steps are
    # rare, and by definition their remaining row updates are at the threshold level: their pose error is bounded at 1e-5.
    hover = ok & ((dA < -1) | (dA > 16))
    print("   residual hovering at the threshold (iteration difference outside [-1, 16]) on %d env-steps, pose err there max %.2e" % (
        hover.sum(), perr[hover].max() if hover.any() else 0.0))
    assert hover.mean() < 2e-3 and (not hover.any() or perr[hover].max() < 1e-5)
    assert (dB != 0).mean() < 5e-3
    assert oerr[ok].max() < 1e-4                                                      # observation (ee position): north_star 1e-3
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# The north_star's acceptance run AS WRITTEN (BASELINE.json): N envs, library defaults, random actions, 1 000
# FREE-RUNNING steps from identical seeds (no resynchronisation), product vs the fp64 oracle at Bullet's exit cadence; per env the first
# step at which the peg-tip position differs by more than 1e-3 m / the contact-normal force by more than 1e-2 N / the observation
# (fingers, end effector: BASELINE.json's "obs L-inf") by more than 1e-3.  The rollout is
# chaotic, so every implementation leaves the oracle's trajectory eventually; the YARDSTICKS say when an fp64 run of
# the ORACLE ITSELF does, under the two perturbations no fp32-state implementation can avoid:
#   Y1  the initial state rounded to fp32 once (sync_oracle(..., rounded=True)), free-running in fp64 afterwards
#   Y2  the state record rounded to fp32 after EVERY step (what the product's 256-word HBM record does to it), Bullet's cadence
#   Y3  as Y2 at the product's exit-test cadence (exit_check_stride = 16)
# and under the perturbation that stands for fp32 ARITHMETIC (the product's one-step error against the oracle from identical inputs is
# 6e-7 m at the median, 2.5e-6 at the 99th percentile -- tests/test_gpu_defaults.py; the probes of ConditionedParity use the same size):
#   Y4  as Y3, and the 77 position / velocity words multiplied by 1 + 1e-6 U(-1, 1) after every step
# In a chaotic rollout the time to leave a tolerance grows with log(tolerance / perturbation): Y2 / Y3 bound what ANY implementation
# with an fp32 state record can reach, Y4 what one with fp32 arithmetic can.
# Reference contract: envs/base_env.py:60-75 driven by env.action_space.sample() (README.md:44-50).
QS = (1, 5, 10, 25, 50, 75, 90)


def _first_exceed(err, tol):
    """err [steps, n] -> first step index with err > tol per env, `steps` where it never happens"""
    ex = err > tol
    return np.where(ex.any(0), ex.argmax(0), err.shape[0])


def _quantiles(first, steps):
    return {"q%02d" % q: int(np.percentile(first, q)) for q in QS} | {"never_share": float((first >= steps).mean()), "min": int(first.min()), "mean": float(first.mean())}


def round_state_fp32(B, rel=0.0, tick=0):
    """fp64 oracle B: pass its state record and warm-start cache through fp32 (what the product's HBM record holds between steps);
    rel > 0: also perturb the 77 position / velocity words by a relative rel * U(-1, 1) (in the oracle library: piho_round_state_fp32)"""
    B.round_state_fp32(rel, 4242, tick)


def first_exceedance_run(oracle_mod, product, N, steps=1000, seed=5, action_seed=8, omp=True, yardsticks=("Y1", "Y2", "Y3", "Y4"), tol_pose=1e-3, tol_force=1e-2, progress=None, product_envs=None):
    """-> dict: per-env first-exceedance steps of the product and of every yardstick (pose, force), their quantiles, and the
    maximum tip / obs difference over the env-steps BEFORE the first exceedance.  `product`: GpuProduct or tests/emul's host build,
    constructed with the same seed, auto_reset as the oracle (library default: off).  product_envs > N: the product steps a LARGER batch
    (its envs are independent and seeded by index) and its first N envs are compared -- the 4096-env launch checked on 1024 of its envs."""
    omp = omp and N >= 64                                  # (a handful of envs: the serial library; thread start-up would dominate)
    A = oracle_mod.Oracle(N, omp=omp, seed=seed)
    Y = {}
    if "Y1" in yardsticks:
        Y["Y1"] = oracle_mod.Oracle(N, omp=omp, seed=seed); sync_oracle(Y["Y1"], A, rounded=True)
    if "Y2" in yardsticks:
        Y["Y2"] = oracle_mod.Oracle(N, omp=omp, seed=seed); round_state_fp32(Y["Y2"])
    if "Y3" in yardsticks:
        Y["Y3"] = oracle_mod.Oracle(N, omp=omp, seed=seed, exit_check_stride=16); round_state_fp32(Y["Y3"])
    if "Y4" in yardsticks:
        Y["Y4"] = oracle_mod.Oracle(N, omp=omp, seed=seed, exit_check_stride=16); round_state_fp32(Y["Y4"])
    # identical seeds: the product's reset state is the oracle's to fp32 rounding (tests: test_reset_matches_oracle)
    M = product_envs or N
    s0 = A.get_state(); sp = product.get_state()[:N]
    assert np.abs(sp[:, POS] - s0[:, POS]).max() < 1e-6
    arng = np.random.default_rng(action_seed + 1)          # actions of the product's extra envs (never compared)
    rng = np.random.default_rng(action_seed)
    names = ["product", *Y]
    perr = {k: np.zeros((steps, N)) for k in names}; ferr = {k: np.zeros((steps, N)) for k in names}; oerr = {k: np.zeros((steps, N)) for k in names}
    ncs = np.zeros((steps, N), dtype=np.int16); fo = np.zeros((steps, N))
    dones = np.zeros(N, dtype=bool)
    for t in range(steps):
        a = rng.uniform(-1, 1, (N, 4))
        oo, _, do = A.step(a); tipA = A.tip_pose()[:, :3]; fA = A.contact_force()
        og, _, dg = product.step(a if M == N else np.concatenate([a, arng.uniform(-1, 1, (M - N, 4))]))
        sg = product.get_state()[:N]; og = np.asarray(og)[:N]
        perr["product"][t] = np.abs(sg[:, _lib.S_TIP : _lib.S_TIP + 3] - tipA).max(1); ferr["product"][t] = np.abs(sg[:, _lib.S_CFORCE] - fA)
        oerr["product"][t] = np.abs(np.asarray(og) - oo).max(1)
        for k, B in Y.items():
            ob, _, _ = B.step(a)
            oerr[k][t] = np.abs(ob - oo).max(1)
            perr[k][t] = np.abs(B.tip_pose()[:, :3] - tipA).max(1); ferr[k][t] = np.abs(B.contact_force() - fA)
            if k != "Y1":
                round_state_fp32(B, 1e-6 if k == "Y4" else 0.0, t + 1)
        ncs[t] = A.ncontacts(); fo[t] = fA; dones |= do.astype(bool)
        if progress and (t + 1) % 100 == 0:
            progress("step %d: product tip err p50 %.2e max %.2e; exceeded so far: %s" % (
                t + 1, np.median(perr["product"][t]), perr["product"][t].max(), {k: int((perr[k][:t + 1] > tol_pose).any(0).sum()) for k in names}))
    out = {"N": N, "product_envs": M, "steps": steps, "seed": seed, "tol_pose_m": tol_pose, "tol_force_N": tol_force, "episodes_ended": int(dones.sum()),
           "mean_contacts": float(ncs.mean()), "max_contacts": int(ncs.max()), "pose": {}, "force": {}, "obs": {}, "first": {}}
    for k in names:
        fp = _first_exceed(perr[k], tol_pose); ff = _first_exceed(ferr[k], tol_force); fb = _first_exceed(oerr[k], tol_pose)
        out["pose"][k] = _quantiles(fp, steps); out["force"][k] = _quantiles(ff, steps); out["obs"][k] = _quantiles(fb, steps)
        out["first"][k] = {"pose": fp, "force": ff, "obs": fb}
    fp = out["first"]["product"]["pose"]
    before = np.arange(steps)[:, None] < fp[None, :]
    out["product_max_tip_err_before_first_exceedance"] = float(perr["product"][before].max()) if before.any() else 0.0
    fb = out["first"]["product"]["obs"]
    before_o = np.arange(steps)[:, None] < fb[None, :]
    out["product_max_obs_err_before_first_exceedance"] = float(oerr["product"][before_o].max()) if before_o.any() else 0.0
    out["product_tip_err_p50_p99_before_first_exceedance"] = [float(np.percentile(perr["product"][before], q)) for q in (50, 99)] if before.any() else [0.0, 0.0]
    out["env_steps_within_tolerance_share"] = {k: float((perr[k] <= tol_pose).mean()) for k in names}
    # what the trajectory was doing when it left: contact count and the oracle's force at the product's first exceedance
    left = fp < steps
    out["contacts_at_first_exceedance_hist"] = np.bincount(ncs[np.minimum(fp, steps - 1)[left], np.nonzero(left)[0]], minlength=1).tolist()
    return out


class ForceLedger:
    """Contact-normal force of two UN-RESYNCHRONISED trajectories (oracle / product), every step held to the north_star's 1e-2 N except
    where the fp64 ORACLE ITSELF moves by more than that: for every step with |dF| > tol / 3 the oracle's step is re-run from 2 K copies
    of ITS input state perturbed by relative 1e-6 / 1e-5 (the two simulations are not in the same state there: by then their
    trajectories differ by ~1e-5 m); the step is a TRANSIENT when any probe's force deviates from the unperturbed one by more than tol (a
    listed contact becomes loaded / unloaded: a 1e-5 m shift decides on which side of the step that happens).  Asserted: |dF| <= tol on every
    non-transient step; |dF| <= K_SPREAD x the probes' largest force deviation on the transients; their share <= `transient_share`; the
    16-step mean <= tol everywhere.  (Round 3 classified by the oracle's own force JUMP and allowed a flat 5e-2 N there.)
        led.before(o); o.step(a); product.step(a); led.after(a, f_oracle, f_product)   ...   led.finish(name)"""
    K, MAGS, K_SPREAD = 16, (1e-6, 1e-5), 10.0

    def __init__(self, oracle_mod, tol=1e-2, slots=256, **cfg):
        cfg.pop("omp", None); cfg.pop("seed", None)
        self.probe = oracle_mod.Oracle(slots, omp=True, **cfg)
        self.slots, self.tol, self.words = slots, tol, oracle_mod.STATE_WORDS
        self.s0, self.c0, self.a, self.fo, self.fg = [], [], [], [], []
        self.rng = np.random.default_rng(777)

    def before(self, o):
        self.s0.append(o.get_state()); self.c0.append(o.warm_cache())

    def after(self, a, fo, fg):
        self.a.append(np.asarray(a, dtype=np.float64).copy()); self.fo.append(np.asarray(fo, dtype=np.float64).copy()); self.fg.append(np.asarray(fg, dtype=np.float64).copy())

    def finish(self, name, skip=0, win=16, transient_share=0.02):
        fo, fg = np.array(self.fo), np.array(self.fg)
        d = np.abs(fo - fg); d[:skip] = 0
        k = np.ones(win) / win
        avg = np.abs(np.stack([np.convolve((fo - fg)[skip:, i], k, mode="valid") for i in range(fo.shape[1])], 1)).max()
        sus = np.argwhere(d > self.tol / 3)
        fdev = np.zeros_like(d)
        rows = [(i, mag) for i in range(len(sus)) for mag in self.MAGS for _ in range(self.K)]
        for c0 in range(0, len(rows), self.slots):
            ch = rows[c0:c0 + self.slots]
            st = np.zeros((self.slots, self.words)); st[:, _lib.S_QUAT + 3] = 1; ac = np.zeros((self.slots, _lib.ACTION_DIM)); ca = np.zeros((self.slots, 97)); ca[:, 1:49] = -1
            for j, (i, mag) in enumerate(ch):
                t, e = sus[i]
                s = self.s0[t][e].copy(); s[:_lib.S_TARGET] *= 1 + mag * self.rng.uniform(-1, 1, _lib.S_TARGET)
                st[j] = s; ac[j] = self.a[t][e]; ca[j] = self.c0[t][e]
            self.probe.set_state(st); self.probe.set_warm_cache(ca); self.probe.step(ac)
            fr = self.probe.contact_force()
            for j, (i, mag) in enumerate(ch):
                t, e = sus[i]
                fdev[t, e] = max(fdev[t, e], abs(fr[j] - fo[t, e]))
        trans = fdev > self.tol
        calm_max = d[~trans].max()
        worst = np.unravel_index(np.argmax(np.where(trans, 0, d)), d.shape)
        over = trans & (d > np.maximum(self.tol, self.K_SPREAD * fdev))
        print("%s: contact force, %d steps x %d envs free-running: |dF| max %.3e N on the %.2f %% of steps where the fp64 oracle's own force is stable under a 1e-6 / 1e-5 perturbation "
              "(bound %.0e); %d transient steps (%.2f %%; the oracle's probes move by up to %.3e N there), |dF| max %.3e N on them; 16-step mean max %.3e N" % (
                  name, d.shape[0], d.shape[1], calm_max, 100 * (~trans).mean(), self.tol, trans.sum(), 100 * trans.mean(), fdev.max(), d[trans].max() if trans.any() else 0.0, avg))
        assert calm_max <= self.tol, "%s: |dF| = %.3e N at step %d env %d where the oracle's own probes move by only %.3e N" % (name, calm_max, worst[0], worst[1], fdev[worst])
        assert not over.any(), "%s: |dF| exceeds %.0f x the oracle's own probe deviation on %d transient steps" % (name, self.K_SPREAD, over.sum())
        assert trans.mean() <= transient_share and avg <= self.tol
        return dict(calm_max=calm_max, transients=int(trans.sum()), avg=avg, inst_max=float(d.max()))


def fly_many_contact_states(sim, n, seed=0):
    """random-fly states with 5 .. 14 contacts (random arm poses lying on the table, the object flat on the table at the end effector): the
    cases beyond the 8 contact records the one-env-per-quad layout keeps in registers (pih_fly.h KR).  sim: anything with get_state /
    set_state / step (oracle.FlyOracle, the host build); it is stepped twice and left in an arbitrary state."""
    rng = np.random.default_rng(seed)
    s = sim.get_state()
    s[:, _lib.F_Q] = rng.uniform(-3, 3, n); s[:, _lib.F_Q + 1] = rng.uniform(-0.3, 0.3, n); s[:, _lib.F_Q + 2] = rng.uniform(-0.5, 0.5, n)
    for k in (3, 4, 5):
        s[:, k] = rng.uniform(-3, 3, n)
    s[:, _lib.F_QD : _lib.F_TARGET] = 0; s[:, _lib.F_DONE] = 0; s[:, _lib.F_STEPS] = 0
    sim.set_state(s); sim.step(np.zeros((n, 6)))
    ee = sim.get_state()[:, _lib.F_EE : _lib.F_CFORCE] - s[:, _lib.F_OFFSET : _lib.F_SPARE]
    s[:, _lib.F_OPOS] = ee[:, 0] + rng.uniform(-0.05, 0.05, n); s[:, _lib.F_OPOS + 1] = ee[:, 1] + rng.uniform(-0.05, 0.05, n); s[:, _lib.F_OPOS + 2] = -0.05 + 0.03
    yaw = rng.uniform(-3, 3, n); s[:, _lib.F_OQUAT] = 0; s[:, _lib.F_OQUAT + 1] = 0; s[:, _lib.F_OQUAT + 2] = np.sin(yaw / 2); s[:, _lib.F_OQUAT + 3] = np.cos(yaw / 2)
    s[:, _lib.F_OVLIN : _lib.F_DONE] = 0
    return s
