#!/usr/bin/env python3
"""Timing of pih_render (wrist camera, 300x300) and pih_grasp_labels for a block of envs.
usage: render_bench.py [n]
       render_bench.py --task random-fly [--n N] --width W --height H [--repeats K]
           the free camera of the random-fly task (pih_render_cam, default camera): float4 flat and shaded, rgba8 flat and shaded, depth,
           float4 and rgba8 with per-env cameras in device memory, alternating with the peg-in-hole wrist camera at the same n and size as
           the yardstick of the same run; stores = 16, 4 and 4 bytes per pixel against the 6.3 TB/s of HBM bandwidth a kernel can reach
           on the MI355X; the last lines compare rgba8 and depth with float4 of the same run
       render_bench.py --task peg-view [--n N] --width W --height H [--repeats K]
           the free camera of the peg-in-hole task (pih_render_view): the wrist preset in float4, rgba8 and depth, the overview camera in
           float4 and rgba8, per-env cameras (the overview in every row) in rgba8, alternating with the unchanged pih_render float4 of
           the same handle as the yardstick of the same run; ms, Mpixel/s and GB/s written for each case
       render_bench.py --task lit [--width W --height H --repeats K]
           the lit images (pih_render_lit) at 1024 and 4096 envs: for each of three shaded yardsticks of the same run -- pih_render_view
           overview, pih_render_view wrist, pih_render_cam default -- the lit call with specular 0 and shadow factor 1 (no shadow ray, no
           highlight), with PIH_LIGHT_DEFAULT but specular 0 (the shadow ray alone), with PIH_LIGHT_DEFAULT, and with PIH_LIGHT_DEFAULT in every row of per-env device lights, in float4 and rgba8; the
           last lines state the cost of the shadow ray + specular term as ratios to the yardstick"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from peg_in_hole_gym_amd import _lib
from peg_in_hole_gym_amd.vec_env import PihVecEnv


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def fly_bench():
    n, W, H, K = _arg("--n", 1024), _arg("--width", 300), _arg("--height", 300), max(5, _arg("--repeats", 5))
    HBM = 6.3e12
    fly = PihVecEnv(n, task_id=1, max_episode_steps=480, contact_margin=0.02, dt=1.0 / 120.0, seed=1)
    act = torch.zeros(n, 6, device="cuda"); act[:, 0] = 0.4; act[:, 2] = 0.5
    fly.step_n(20, act)                          # objects in flight, arms off their rest pose
    peg = PihVecEnv(n, mode=1, dv=0.05)
    peg.step_n(540)
    out = torch.empty(n, H, W, 4, device="cuda")
    out8 = torch.empty(n, H, W, 4, dtype=torch.uint8, device="cuda")
    outd = torch.empty(n, H, W, device="cuda")
    cams = torch.tensor([_lib.FLY_CAM_DEFAULT] * n, device="cuda")      # per-env cameras in device memory: the default camera in every row, so the pixels are the same work
    # (name, bytes stored per pixel, call); "float4 flat" is pih_fly_image_kernel<0> with one host camera, like every other case without per-env cameras
    cases = (("random-fly float4 flat", 16, lambda: fly.render(W, H, out=out)),
             ("random-fly float4 shaded", 16, lambda: fly.render(W, H, out=out, shaded=True)),
             ("random-fly rgba8 flat", 4, lambda: fly.render(W, H, out=out8, fmt="rgba8")),
             ("random-fly rgba8 shaded", 4, lambda: fly.render(W, H, out=out8, fmt="rgba8", shaded=True)),
             ("random-fly depth", 4, lambda: fly.render(W, H, out=outd, fmt="depth")),
             ("random-fly float4 flat, per-env cameras", 16, lambda: fly.render(W, H, out=out, camera=cams)),
             ("random-fly rgba8 flat, per-env cameras", 4, lambda: fly.render(W, H, out=out8, fmt="rgba8", camera=cams)),
             ("peg-in-hole float4 flat", 16, lambda: peg.render(W, H, out=out)))
    for _, _, f in cases:                        # warm-up
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in cases}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(K):                           # alternating: every repeat times each case once
        for name, _, f in cases:
            ev[0].record(); f(); ev[1].record(); ev[1].synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    for name, bpp, _ in cases:
        v = sorted(ms[name]); med = v[len(v) // 2]
        print("%-40s %d envs x %dx%d: median %.3f ms (min %.3f, max %.3f, %d repeats) = %.0f images/s, %.0f Mpixel/s, %d B/pixel stored: %.2f TB/s = %.0f %% of 6.3 TB/s"
              % (name, n, W, H, med, v[0], v[-1], K, n / (med * 1e-3), n * W * H / med / 1e3, bpp, n * W * H * bpp / med / 1e9, 100 * n * W * H * bpp / (med * 1e-3) / HBM))
    ref = sorted(ms["random-fly float4 flat"]); spread = ref[-1] - ref[0]
    for name in ("random-fly rgba8 flat", "random-fly depth"):
        med = sorted(ms[name])[K // 2]
        print("%-40s median %.3f ms vs float4 flat %.3f ms + its spread %.3f ms: %s" % (name, med, ref[K // 2], spread, "within" if med <= ref[K // 2] + spread else "SLOWER"))


def peg_view_bench():
    n, W, H, K = _arg("--n", 1024), _arg("--width", 300), _arg("--height", 300), max(5, _arg("--repeats", 5))
    peg = PihVecEnv(n, mode=1, dv=0.05)
    peg.step_n(540)                              # grippers hovering above their pipes, as in the default timing
    out = torch.empty(n, H, W, 4, device="cuda")
    out8 = torch.empty(n, H, W, 4, dtype=torch.uint8, device="cuda")
    outd = torch.empty(n, H, W, device="cuda")
    over = _lib.VIEW_CAM_OVERVIEW
    cams = torch.tensor([over] * n, device="cuda")      # per-env cameras in device memory: the overview in every row, so the pixels are the same work
    cases = (("pih_render float4 (wrist, yardstick)", 16, lambda: peg.render(W, H, out=out)),
             ("view wrist float4", 16, lambda: peg.render_view(W, H, out=out)),
             ("view wrist rgba8", 4, lambda: peg.render_view(W, H, out=out8, fmt="rgba8")),
             ("view wrist depth", 4, lambda: peg.render_view(W, H, out=outd, fmt="depth")),
             ("view overview float4", 16, lambda: peg.render_view(W, H, out=out, camera=over)),
             ("view overview rgba8", 4, lambda: peg.render_view(W, H, out=out8, camera=over, fmt="rgba8")),
             ("view overview rgba8, per-env cameras", 4, lambda: peg.render_view(W, H, out=out8, camera=cams, fmt="rgba8")))
    for _, _, f in cases:                        # warm-up
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in cases}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(K):                           # alternating: every repeat times each case once
        for name, _, f in cases:
            ev[0].record(); f(); ev[1].record(); ev[1].synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    ref = sorted(ms[cases[0][0]])[K // 2]
    for name, bpp, _ in cases:
        v = sorted(ms[name]); med = v[len(v) // 2]
        print("%-40s %d envs x %dx%d: median %.3f ms (min %.3f, max %.3f, %d repeats) = %.0f Mpixel/s, %d B/pixel stored: %.1f GB/s written, %.2f x the yardstick's time"
              % (name, n, W, H, med, v[0], v[-1], K, n * W * H / med / 1e3, bpp, n * W * H * bpp / med / 1e6, med / ref))


def lit_bench():
    W, H, K = _arg("--width", 300), _arg("--height", 300), max(5, _arg("--repeats", 5))
    off = list(_lib.LIGHT_DEFAULT); off[8] = 0.0; off[10] = 1.0          # specular 0, shadow factor 1
    matt = list(_lib.LIGHT_DEFAULT); matt[8] = 0.0                        # specular 0: the shadow ray alone
    for n in (1024, 4096):
        peg = PihVecEnv(n, mode=1, dv=0.05)
        peg.step_n(540)                          # grippers hovering above their pipes, as in the default timing
        fly = PihVecEnv(n, task_id=1, max_episode_steps=480, contact_margin=0.02, dt=1.0 / 120.0, seed=1)
        act = torch.zeros(n, 6, device="cuda"); act[:, 0] = 0.4; act[:, 2] = 0.5
        fly.step_n(20, act)                      # objects in flight, arms off their rest pose
        out = torch.empty(n, H, W, 4, device="cuda")
        out8 = torch.empty(n, H, W, 4, dtype=torch.uint8, device="cuda")
        lights = torch.tensor([_lib.LIGHT_DEFAULT] * n, device="cuda")      # per-env lights in device memory: the default in every row, so the pixels are the same work
        scenes = (("view overview", lambda **kw: peg.render_view(W, H, camera=_lib.VIEW_CAM_OVERVIEW, **kw)),
                  ("view wrist", lambda **kw: peg.render_view(W, H, **kw)),
                  ("fly default", lambda **kw: fly.render(W, H, **kw)))
        cases = []
        for sname, f in scenes:
            for fmt, o, bpp in (("float4", out, 16), ("rgba8", out8, 4)):
                cases.append((sname, fmt, "shaded (yardstick)", bpp, lambda f=f, fmt=fmt, o=o: f(out=o, fmt=fmt, shaded=True)))
                cases.append((sname, fmt, "lit, specular 0, shadow 1", bpp, lambda f=f, fmt=fmt, o=o: f(out=o, fmt=fmt, light=off)))
                cases.append((sname, fmt, "lit, default but specular 0", bpp, lambda f=f, fmt=fmt, o=o: f(out=o, fmt=fmt, light=matt)))
                cases.append((sname, fmt, "lit, default light", bpp, lambda f=f, fmt=fmt, o=o: f(out=o, fmt=fmt, light="default")))
                cases.append((sname, fmt, "lit, default, per-env lights", bpp, lambda f=f, fmt=fmt, o=o: f(out=o, fmt=fmt, light=lights)))
        for c in cases:                          # warm-up
            for _ in range(2):
                c[4]()
        torch.cuda.synchronize()
        ms = {c[:3]: [] for c in cases}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(K):                       # alternating: every repeat times each case once
            for c in cases:
                ev[0].record(); c[4](); ev[1].record(); ev[1].synchronize()
                ms[c[:3]].append(ev[0].elapsed_time(ev[1]))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        for sname, fmt, what, bpp, _ in cases:
            v = sorted(ms[(sname, fmt, what)]); m = med[(sname, fmt, what)]
            print("%-14s %-6s %-30s %d envs x %dx%d: median %.3f ms (min %.3f, max %.3f, %d repeats) = %.0f Mpixel/s, %.1f GB/s written, %.2f x the yardstick's time"
                  % (sname, fmt, what, n, W, H, m, v[0], v[-1], K, n * W * H / m / 1e3, n * W * H * bpp / m / 1e6, m / med[(sname, fmt, "shaded (yardstick)")]))
        for sname, _ in scenes:
            for fmt in ("float4", "rgba8"):
                y, a, b = med[(sname, fmt, "shaded (yardstick)")], med[(sname, fmt, "lit, specular 0, shadow 1")], med[(sname, fmt, "lit, default light")]
                m = med[(sname, fmt, "lit, default but specular 0")]
                print("%-14s %-6s %d envs: lit kernel without shadow ray and highlight %.2f x the shaded yardstick; the shadow ray adds %.2f x, the specular term %.2f x the yardstick"
                      % (sname, fmt, n, a / y, (m - a) / y, (b - m) / y))
        del peg, fly


if "--task" in sys.argv:
    task = _arg("--task", "")
    if task not in ("random-fly", "peg-view", "lit"):
        sys.exit("render_bench.py: --task takes random-fly, peg-view or lit (the peg-in-hole wrist camera timing is the default: render_bench.py [n])")
    {"random-fly": fly_bench, "peg-view": peg_view_bench, "lit": lit_bench}[task]()
    sys.exit(0)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
g = PihVecEnv(n, mode=1, dv=0.05)
g.step_n(540)
out = torch.empty(n, 300, 300, 4, device="cuda")
for _ in range(2):
    g.render(300, 300, out=out)
torch.cuda.synchronize()
t0 = time.perf_counter()
K = 5
for _ in range(K):
    g.render(300, 300, out=out)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / K
print("render: %d envs x 300x300 in %.3f ms = %.1f Mpixel/s, %.1f GB/s written, %.0f images/s" % (n, dt * 1e3, n * 9e4 / dt / 1e6, n * 9e4 * 16 / dt / 1e9, n / dt))
g.step_n(1)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(K):
    lab, meta = g.grasp_labels(300)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / K
print("labels: %d envs x 4x300x300 in %.3f ms = %.1f GB/s written" % (n, dt * 1e3, n * 9e4 * 16 / dt / 1e9))
