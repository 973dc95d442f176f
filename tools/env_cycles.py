"""Diagnostic: per-env shader-clock cycles of pih_step_kernel (config.debug = 2 stamps) by contact count, for both PGS paths.
usage: python tools/env_cycles.py [n_envs]      Not a benchmark (the stamps cost ~10 %)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from peg_in_hole_gym_amd import _lib
from peg_in_hole_gym_amd.vec_env import PihVecEnv
CYC = _lib.DBG_CYCLES            # + k: cycles of phase k (0 .. 7; 5 = PGS)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
sched = int(sys.argv[2]) if len(sys.argv) > 2 else 1
for path in (0, 1):
    env = PihVecEnv(n, auto_reset=1, debug=2, solver_path=path, max_episode_steps=2227, schedule=sched)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    tot = []; pgs = []; cnt = []; smax = []; sarg = []; sph = []; phs = []; col = []
    for t in range(460):
        env.step(torch.rand(n, 4, device="cuda", generator=gen) * 2 - 1)
        if t >= 400 and t % 5 == 0:
            d = env.debug()
            col.append(d[:, CYC + 17:CYC + 22].clone())
            tot.append(d[:, CYC:CYC + 8].sum(1)); pgs.append(d[:, CYC + 5]); cnt.append(env.state()[:, _lib.S_NCONTACT]); phs.append(d[:, CYC:CYC + 8].clone())
            i = int(tot[-1].argmax()); smax.append(float(tot[-1][i])); sarg.append(int(cnt[-1][i])); sph.append(d[i, CYC:CYC + 8].tolist())
    tot = torch.cat(tot); pgs = torch.cat(pgs); cnt = torch.cat(cnt); phs = torch.cat(phs); col = torch.cat(col)
    q = lambda x, p: float(torch.quantile(x.float(), p))
    print("solver_path %d: per-env cycles mean %.0f p50 %.0f p90 %.0f p99 %.0f max %.0f | PGS mean %.0f | mean contacts %.2f | sum/2048 slots %.0f" % (
        path, tot.mean(), q(tot, .5), q(tot, .9), q(tot, .99), tot.max(), pgs.mean(), cnt.mean(), tot.sum() / len(tot) * n / 2048))
    print("   heaviest env of a step (the launch cannot end before it does): mean %.0f cycles, min %.0f, max %.0f; its contacts: mean %.1f min %d max %d" % (
        sum(smax) / len(smax), min(smax), max(smax), sum(sarg) / len(sarg), min(sarg), max(sarg)))
    ph = torch.tensor(sph).mean(0).tolist()
    print("   its phases: fk %.0f fsm %.0f collide %.0f aba %.0f rows %.0f pgs %.0f integrate %.0f fk2 %.0f" % tuple(ph))
    for lo, hi in ((0, 4), (5, 7), (8, 10), (11, 14), (15, 19), (20, 24), (25, 32), (33, 48)):
        m = (cnt >= lo) & (cnt <= hi)
        if m.any():
            print("   contacts %2d..%2d: %5.1f %% of env-steps, total %.0f cycles, PGS %.0f; phases fk %.0f fsm %.0f collide %.0f aba %.0f rows %.0f pgs %.0f integrate %.0f fk2 %.0f" % (
                (lo, hi, 100 * m.float().mean(), tot[m].mean(), pgs[m].mean()) + tuple(phs[m].mean(0).tolist())))
            # stamps 17 .. 21 inside collide (include/pih.h; the rest of the phase: its entry and the stamps themselves)
            print("      collide: constants + samples + candidates %.0f | slots of table, tube, attach, weld, arm spheres vs table %.0f | of the pads %.0f | of arm spheres vs pipe %.0f | pairs %.0f" % tuple(col[m].mean(0).tolist()))
