"""Inputs, reference and comparison rule of the batched closest-point queries (pih_closest_points), CPU and GPU: tests/test_dist.py and
tests/test_gpu_dist.py.  The reference is the fp64 numpy signed distance of every primitive of the scenes of tests/render_ref.py
(peg_scene, fly_scene) below; the host builds of the product's per-query code are bound in tests/emul/dist_emul.py.

States: those of tests/ray_cases.py (peg-in-hole: the six of render_cases.make_view_states; random-fly: three per object).

Query families (rounded to float32 here, so every build and the reference see the same numbers):
  near        1024 queries per state from rng(500 + state index): a quarter uniform in ray_cases.BOX_LO .. BOX_HI, the rest a random
              primitive's anchor (as ray_cases.aimed_rays picks it; the table: a point of the plane under the box) + N(0, 0.03); every
              fourth query has reach 0.05, the rest 10.  Run with all groups and (peg-in-hole) without arm and fingers
  group       per single group of the task 512 queries from rng(800 + 10 x state index + group): a random primitive of the group, its
              anchor + N(0, its radius / smallest half-extent; tube 0.01; table 0.03), reaches as above, run with that group alone.
              (The near family against the pipe alone has up to 0.37 of its queries nearest to a vertex two capsules share -- from afar
              the outside of every bend is -- which is over the cap below; within a radius of the pipe the share is smaller.)
  hole        (peg-in-hole) 768 queries in cylinder coordinates about the hole's axis: a third uniform in the box +-(0.032, 0.035, 0.035)
              about PIH_HOLE_POS; a third with rho uniform in [rin - 2 mm, rout + 2 mm] and |x| <= halflen + 2 mm; a third in the bore.
              Run against the hole alone and against all groups
  inside      per primitive 8 queries at its anchor + N(0, 0.4 x its radius / smallest half-extent / half wall thickness), run with that
              primitive's group alone
  degenerate  sphere centres, capsule-axis midpoints and end points, the hole's centre and points of its axis, a point on the table
              plane: where the closest point is not unique.  Run with every single group and with all.  (Every vertex of the pipe and
              the arm is shared by two capsules: the cap on queries with more than one seg does not apply to this family.)
  ee          a 5 x 5 x 5 lattice of +-5 cm in the end-effector frame, PIH_RAY_FRAME_EE, all groups

Rule at tolerance G, per query (judge):
  1. the reference distance d_i of every selected primitive; dmin the smallest; N = the primitives with d_i <= dmin + 2 G
  2. dmin > reach + G: the record must be the miss record (reach | SEG_NONE | the query point, env-local | 0); dmin < reach - G: it must
     be a hit; in between either
  3. a hit: |w0 - dmin| <= G; the seg is that of a member of N; the position lies on that primitive, |d_i(pos)| <= G; | |n| - 1 | <= 1e-5;
     |p - (pos + w0 n)| <= 2 G
  4. where |w0| < 1e-4 check 3's last line cannot see n: there n is compared with the reference's outward normal at pos, to 1e-3, leaving
     out positions within 1e-4 of a box or tube edge -- at most 1 % of a case's queries
Conditions on the reference, asserted by check_families (conditions on the inputs, not tolerances): near with all groups: share of negative
distances >= 0.1, of positive ones >= 0.3, among the reach = 0.05 queries both outcomes >= 0.1; every seg of ray_cases.reachable_segs
except peg-in-hole arm links 1 and 5 (link 1's capsule has zero length and sits on link 0's end, link 5 lies inside its neighbours) is the
unique member of N for >= 3 near queries over the states; at most 0.25 of a case's queries have more than one seg in N at G_GPU
(neighbouring pipe and arm capsules share end spheres); hole: inside the wall >= 0.1, in the bore >= 0.25, beyond an end face >= 0.1;
inside: per finger box and for the tube >= 3 queries with distance < -1 mm.

G is measured, by the protocol of tests/ray_cases.py.  G_HOST is the smallest value of ray_cases.G_GRID at which the fp32 HOST build
(g++ -O2 -fno-fast-math) passes every case; the GPU tests use G_GPU, two grid steps above it; never more than render_ref.DELTA.  The
fp64 host build passes at G_F64 = 1e-9.  Measured with measure_host() (python -m tests.dist_cases) on 2026-10-21:
  G_HOST = 1e-6, the grid's smallest value: the fp32 host build passes all 186 cases; largest use of G 0.152 (the largest of
           |w0 - dmin|, |d_i(pos)| and |p - (pos + w0 n)| / 2 over all hits, as a share of G; 0.030 at G_GPU = 5e-6).  Rule 4 leaves out at
           most 0.0013 of a case's queries; at most 0.234 of a case's queries have more than one seg in N at G_GPU (near, without arm
           and fingers; all groups: 0.106).  Before sd_capsule took the rounding's axial part out of the normal, the degenerate family's
           positions were up to 2.5e-2 m off the surface at every G of the grid.
  GPU (one MI355X, 2026-10-21, one box, one run, tests/test_gpu_dist.py): largest use of G_GPU 0.092 (peg-in-hole), 0.029 / 0.035
           (random-fly, the two objects) over all sizes, env ranges, groups and frames -- the GPU's share of G_GPU, 4.6e-7 m at most.
"""
import numpy as np

from peg_in_hole_gym_amd import _lib
from tests import ray_cases as RY
from tests import render_cases as RC
from tests import render_ref as R

G_F64 = 1e-9
G_HOST = 1e-6
G_GPU = RY.G_GRID[RY.G_GRID.index(G_HOST) + 2]
assert G_GPU <= R.DELTA
N_NEAR, N_GROUP, N_HOLE, N_INSIDE = 1024, 512, 768, 8
SIGMA_NEAR = 0.03
REACH_FAR, REACH_NEAR = 10.0, 0.05
SMALL_DISTANCE = 1e-4           # below it the normal is compared with the reference's (rule 4)
EDGE = 1e-4                     # ... unless the position is this close to a box or tube edge
NORMAL_TOL = 1e-3
LEFT_OUT_CAP = 0.01
MULTI_SEG_CAP = 0.25
W_DIST, W_SEG, W_POS, W_NORMAL = 0, 1, 2, 5
TABLE = "table"                 # the pseudo-primitive of the table plane


# ------------------------------------------------------------------------------------------------ reference signed distances
def _box2(x, h):
    """signed distance of the box |x_k| <= h_k (x [N, K], h [K]): Euclidean outside, -(distance to the nearest face) inside"""
    q = np.abs(x) - h
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)


def _axis_point(pr, p):
    a, b = pr.p["a"], pr.p["b"]
    ba = b - a
    t = np.clip(((p - a) @ ba) / max(ba @ ba, 1e-300), 0.0, 1.0)
    return a + t[:, None] * ba


def _tube_coords(p):
    oc = p - R.HOLE_POS
    return oc[:, 0], np.hypot(oc[:, 1], oc[:, 2])


def signed_distance(scene, pr, p):
    """fp64 signed distance of the points p [N, 3] (env-local) to one primitive (a render_ref.Prim or TABLE)"""
    if pr is TABLE:
        return p[:, 2] - scene.table_z
    if pr.kind == "sphere":
        return np.linalg.norm(p - pr.p["c"], axis=1) - pr.p["r"]
    if pr.kind == "capsule":
        return np.linalg.norm(p - _axis_point(pr, p), axis=1) - pr.p["r"]
    if pr.kind == "box":
        return _box2((p - pr.p["c"]) @ pr.p["R"], pr.p["h"])
    hl, rin, rout = R._tube(0.0)
    ax, rho = _tube_coords(p)
    return _box2(np.stack([ax, rho - 0.5 * (rin + rout)], 1), np.array([hl, 0.5 * (rout - rin)]))


def surface_normal(scene, pr, pos):
    """the outward unit normal of the primitive at the surface points pos [N, 3] -> (n [N, 3], near_edge [N]: within EDGE of a box or tube edge)"""
    N = len(pos)
    edge = np.zeros(N, bool)
    if pr is TABLE:
        return np.tile([0.0, 0.0, 1.0], (N, 1)), edge
    if pr.kind == "sphere":
        return R._radial(pos, pr.p["c"]), edge
    if pr.kind == "capsule":
        return R._radial(pos, _axis_point(pr, pos)), edge
    if pr.kind == "box":
        x = (pos - pr.p["c"]) @ pr.p["R"]
        q = np.abs(x) - pr.p["h"]
        face = q.argmax(1)
        nl = np.zeros((N, 3)); nl[np.arange(N), face] = np.where(x[np.arange(N), face] < 0, -1.0, 1.0)
        return nl @ pr.p["R"].T, (np.abs(q) < EDGE).sum(1) >= 2
    hl, rin, rout = R._tube(0.0)
    oc = pos - R.HOLE_POS
    ax, rho = _tube_coords(pos)
    q = np.stack([np.abs(ax) - hl, np.abs(rho - 0.5 * (rin + rout)) - 0.5 * (rout - rin)], 1)
    e = np.stack([np.zeros(N), oc[:, 1], oc[:, 2]], 1) / np.maximum(rho, 1e-300)[:, None]
    n = np.where((q[:, 0] >= q[:, 1])[:, None], np.stack([np.where(ax < 0, -1.0, 1.0), np.zeros(N), np.zeros(N)], 1),
                 np.where(rho < 0.5 * (rin + rout), -1.0, 1.0)[:, None] * e)
    return n, (np.abs(q) < EDGE).sum(1) >= 2


# ------------------------------------------------------------------------------------------------ groups
def group_of(scene, pr):
    if pr is TABLE:
        return _lib.GROUP_TABLE
    if scene.task == "peg":
        if pr.seg <= R.SEG_HAND:
            return _lib.GROUP_ARM
        if pr.seg <= R.SEG_FINGER0 + 1:
            return _lib.GROUP_FINGERS
        return _lib.GROUP_HOLE if pr.seg == _lib.VIEW_SEG_HOLE else _lib.GROUP_OBJECT
    return _lib.GROUP_ARM if pr.seg < _lib.SEG_OBJECT else _lib.GROUP_OBJECT


def seg_of(scene, pr):
    return scene.table[1] if pr is TABLE else pr.seg


def selected(scene, groups):
    """the primitives `groups` selects, the table first (its place in the product's walk)"""
    return [pr for pr in [TABLE] + list(scene.prims) if group_of(scene, pr) & groups]


def task_groups(task):
    """the single groups a task has"""
    if task == "peg":
        return (_lib.GROUP_ARM, _lib.GROUP_FINGERS, _lib.GROUP_OBJECT, _lib.GROUP_HOLE, _lib.GROUP_TABLE)
    return (_lib.GROUP_ARM, _lib.GROUP_OBJECT, _lib.GROUP_TABLE)


# ------------------------------------------------------------------------------------------------ families
def _f32(a):
    return np.asarray(a, dtype=np.float32)


def anchor(scene, pr, rng):
    """a point of the primitive's inside, as ray_cases.aimed_rays picks it; the table: a point of the plane under the box"""
    if pr is TABLE:
        a = rng.uniform(RY.BOX_LO, RY.BOX_HI); a[2] = scene.table_z
        return a
    if pr.kind == "capsule":
        return pr.p["a"] + rng.uniform() * (pr.p["b"] - pr.p["a"])
    if pr.kind in ("sphere", "box"):
        return pr.p["c"]
    v = rng.normal(size=3)
    return R.HOLE_POS + 0.02 * rng.uniform() ** (1 / 3) * v / np.linalg.norm(v)


def _with_reach(xyz):
    reach = np.where(np.arange(len(xyz)) % 4 == 0, REACH_NEAR, REACH_FAR)
    return _f32(np.concatenate([xyz, reach[:, None]], axis=1))


def near_points(scene, index):
    """float32 [N_NEAR, 4] of the near family for the scene of state `index`"""
    rng = np.random.default_rng(500 + index)
    n, q = N_NEAR, N_NEAR // 4
    prims = [TABLE] + list(scene.prims)
    xyz = np.empty((n, 3))
    xyz[:q] = rng.uniform(RY.BOX_LO, RY.BOX_HI, (q, 3))
    for i in range(q, n):
        xyz[i] = anchor(scene, prims[rng.integers(len(prims))], rng) + rng.normal(0.0, SIGMA_NEAR, 3)
    return _with_reach(xyz[rng.permutation(n)])


def group_points(scene, index, group):
    """float32 [N_GROUP, 4] around the primitives of one group"""
    rng = np.random.default_rng(800 + 10 * index + group)
    prims = selected(scene, group)
    xyz = np.empty((N_GROUP, 3))
    for i in range(N_GROUP):
        pr = prims[rng.integers(len(prims))]
        sigma = 0.03 if pr is TABLE else (0.01 if pr.kind == "tube" else scale_of(pr))
        xyz[i] = anchor(scene, pr, rng) + rng.normal(0.0, sigma, 3)
    return _with_reach(xyz)


def hole_points(index):
    """float32 [N_HOLE, 4] about the hole tube"""
    rng = np.random.default_rng(600 + index)
    hl, rin, rout = R._tube(0.0)
    t = N_HOLE // 3
    box = rng.uniform(-1.0, 1.0, (t, 3)) * [0.032, 0.035, 0.035]

    def cyl(x, rho):
        phi = rng.uniform(0, 2 * np.pi, len(x))
        return np.stack([x, rho * np.cos(phi), rho * np.sin(phi)], 1)

    wall = cyl(rng.uniform(-hl - 0.002, hl + 0.002, t), rng.uniform(rin - 0.002, rout + 0.002, t))
    bore = cyl(rng.uniform(-hl, hl, t), rin * rng.uniform(0.0, 0.98, t))
    return _with_reach(R.HOLE_POS + np.concatenate([box, wall, bore])[rng.permutation(3 * t)])


def scale_of(pr):
    """radius / smallest half-extent / half wall thickness"""
    if pr.kind in ("sphere", "capsule"):
        return pr.p["r"]
    if pr.kind == "box":
        return float(np.min(pr.p["h"]))
    hl, rin, rout = R._tube(0.0)
    return 0.5 * (rout - rin)


def inside_points(scene, index, group):
    """float32 [8 x primitives of the group, 4]; the tube's anchor lies in its wall"""
    rng = np.random.default_rng(700 + 10 * index + group)
    hl, rin, rout = R._tube(0.0)
    rows = []
    for pr in scene.prims:
        if group_of(scene, pr) != group:
            continue
        for _ in range(N_INSIDE):
            if pr.kind == "tube":
                phi = rng.uniform(0, 2 * np.pi)
                a = R.HOLE_POS + [rng.uniform(-0.8, 0.8) * hl, 0.5 * (rin + rout) * np.cos(phi), 0.5 * (rin + rout) * np.sin(phi)]
            else:
                a = anchor(scene, pr, rng)
            rows.append(a + rng.normal(0.0, 0.4 * scale_of(pr), 3))
    return _f32(np.concatenate([np.array(rows), np.full((len(rows), 1), REACH_FAR)], axis=1))


def degenerate_points(scene):
    rows = []
    for pr in scene.prims:
        if pr.kind == "sphere":
            rows.append(pr.p["c"])
        elif pr.kind == "capsule":
            rows += [0.5 * (pr.p["a"] + pr.p["b"]), pr.p["a"], pr.p["b"]]
        elif pr.kind == "tube":
            hl = R._tube(0.0)[0]
            rows += [R.HOLE_POS, R.HOLE_POS + [0.5 * hl, 0, 0], R.HOLE_POS + [hl + 0.004, 0, 0], R.HOLE_POS - [hl, 0, 0]]
    rows.append(np.array([0.1, -0.7, scene.table_z]))
    return _f32(np.concatenate([np.array(rows), np.full((len(rows), 1), REACH_FAR)], axis=1))


def ee_points():
    g = np.linspace(-0.05, 0.05, 5)
    return _with_reach(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def make_cases(O):
    """[case]: dict(task, obj, state (index among the task's states), rec float32, scene, name, points float32 [N, 4], frame "env" | "ee",
    groups, flags)"""
    cases = []

    def add(task, obj, k, rec, scene, name, points, frame, groups):
        cases.append(dict(task=task, obj=obj, state=k, rec=rec, scene=scene, name=name, points=points, frame=frame, groups=groups,
                          flags=_lib.RAY_FRAME_EE if frame == "ee" else 0))

    def family(task, obj, k, rec, scene, index):
        near, deg = near_points(scene, index), degenerate_points(scene)
        add(task, obj, k, rec, scene, "near", near, "env", _lib.GROUP_ALL)
        for groups in (_lib.GROUP_ALL,) + task_groups(task):
            add(task, obj, k, rec, scene, "degenerate", deg, "env", groups)
        for group in task_groups(task):
            add(task, obj, k, rec, scene, "group", group_points(scene, index, group), "env", group)
            if group != _lib.GROUP_TABLE:
                add(task, obj, k, rec, scene, "inside", inside_points(scene, index, group), "env", group)
        add(task, obj, k, rec, scene, "ee", ee_points(), "ee", _lib.GROUP_ALL)

    for k, rec in enumerate(RC.make_view_states(O)):
        scene = R.peg_scene(O, rec)
        family("peg", None, k, rec, scene, k)
        add("peg", None, k, rec, scene, "near", near_points(scene, k), "env", _lib.GROUP_ALL & ~(_lib.GROUP_ARM | _lib.GROUP_FINGERS))
        for groups in (_lib.GROUP_HOLE, _lib.GROUP_ALL):
            add("peg", None, k, rec, scene, "hole", hole_points(k), "env", groups)
    for obj in RC.OBJECTS:
        for k, rec in enumerate(RC.make_fly_states(O, obj, RY.FLY_STATES_PER_OBJECT, RY.FLY_SEED[obj])):
            family("fly", obj, k, rec, R.fly_scene(O, rec, obj), 10 + RY.FLY_STATES_PER_OBJECT * obj + k)
    return cases


def case_id(c):
    return "%s%s-%d-%s-g%d" % (c["task"], "" if c["obj"] is None else c["obj"], c["state"], c["name"], c["groups"])


# ------------------------------------------------------------------------------------------------ reference and rule
def env_points(scene, points, frame):
    """queries float32 [N, 4] -> (p [N, 3] env-local fp64, reach [N])"""
    w = np.asarray(points, dtype=np.float32).astype(np.float64)
    p = w[:, :3]
    if frame == "ee":
        pe, Re = scene.ee
        p = pe + p @ Re.T
    assert np.isfinite(w).all() and (w[:, 3] > 0).all(), "a bad query among the queries of a family"
    return p, w[:, 3]


def expected(case):
    """-> dict: p, reach, prims (the selected ones), segs [K], D [K, N] reference distances, dmin [N]"""
    scene = case["scene"]
    p, reach = env_points(scene, case["points"], case["frame"])
    prims = selected(scene, case["groups"])
    assert prims, "the groups of %s select nothing" % case_id(case)
    D = np.stack([signed_distance(scene, pr, p) for pr in prims])
    return dict(p=p, reach=reach, prims=prims, segs=np.array([seg_of(scene, pr) for pr in prims]), D=D, dmin=D.min(0))


def multi_seg_share(e, G):
    near = e["D"] <= e["dmin"] + 2 * G
    return float(np.mean([len(set(e["segs"][near[:, j]])) > 1 for j in range(near.shape[1])]))


def judge(case, G, out, exp=None):
    """a build's records out [N, 8] against the rule -> dict(fail: {what: number of queries}, use: the largest share of G a hit uses,
    left_out: share of the queries rule 4 leaves out)"""
    e = expected(case) if exp is None else exp
    scene = case["scene"]
    out = np.asarray(out, dtype=np.float64)
    N = len(out)
    assert out.shape == (N, 8) and N == len(e["p"])
    w0, seg, pos, n = out[:, W_DIST], out[:, W_SEG], out[:, W_POS:W_POS + 3], out[:, W_NORMAL:W_NORMAL + 3]
    p, reach, dmin = e["p"], e["reach"], e["dmin"]
    fail = {}
    fail["finite"] = int((~np.isfinite(out).all(1)).sum())
    is_miss = seg == _lib.SEG_NONE
    fail["hit where a miss is due"] = int((~is_miss & (dmin > reach + G)).sum())
    fail["miss where a hit is due"] = int((is_miss & (dmin < reach - G)).sum())
    fail["miss record"] = int((is_miss & ~((w0 == reach) & (np.abs(pos - p).max(1) <= G) & (n == 0).all(1))).sum())
    hit = ~is_miss & np.isfinite(out).all(1)
    fail["distance"] = int((hit & ~(np.abs(w0 - dmin) <= G)).sum())
    # the member of N the record names: of the selected primitives with the record's seg and d_i <= dmin + 2 G, the one the position is nearest to
    on = np.full(N, np.inf); member = np.full(N, -1)
    for i, pr in enumerate(e["prims"]):
        m = hit & (seg == e["segs"][i]) & (e["D"][i] <= dmin + 2 * G)
        if m.any():
            d = np.abs(signed_distance(scene, pr, pos[m]))
            better = d < on[m]
            idx = np.flatnonzero(m)[better]
            on[idx] = d[better]; member[idx] = i
    fail["seg"] = int((hit & (member < 0)).sum())
    named = hit & (member >= 0)
    fail["position"] = int((named & ~(on <= G)).sum())
    fail["unit normal"] = int((hit & ~(np.abs(np.linalg.norm(n, axis=1) - 1) <= 1e-5)).sum())
    back = np.linalg.norm(p - (pos + w0[:, None] * n), axis=1)
    fail["p = pos + d n"] = int((hit & ~(back <= 2 * G)).sum())
    small = named & (np.abs(w0) < SMALL_DISTANCE)
    left_out = np.zeros(N, bool); wrong = np.zeros(N, bool)
    for i in np.unique(member[small]):
        m = np.flatnonzero(small & (member == i))
        nref, edge = surface_normal(scene, e["prims"][i], pos[m])
        left_out[m] = edge
        wrong[m] = ~edge & (np.abs(n[m] - nref).max(1) > NORMAL_TOL)
    fail["normal at a small distance"] = int(wrong.sum())
    fail["left out"] = int(left_out.sum()) if left_out.mean() > LEFT_OUT_CAP else 0
    use = np.maximum(np.abs(w0 - dmin), np.maximum(np.where(np.isfinite(on), on, 0.0), 0.5 * back))[named]
    return dict(fail={k: v for k, v in fail.items() if v}, use=float(use.max() / G) if len(use) else 0.0, left_out=float(left_out.mean()))


def check(case, G, out, exp=None):
    res = judge(case, G, out, exp)
    assert not res["fail"], "%s at G = %g: queries that break the rule: %s (largest use of G %.3f)" % (case_id(case), G, res["fail"], res["use"])
    return res


def check_families(cases, G):
    """the conditions on the reference (module docstring); the multi-seg share at G"""
    unique = {}
    inside_deep = {}
    for c in cases:
        e = expected(c)
        share = multi_seg_share(e, G)
        assert share <= MULTI_SEG_CAP or c["name"] == "degenerate", "%s: %.3f of the queries have more than one seg within 2 G = %g" % (case_id(c), share, 2 * G)
        dmin, reach = e["dmin"], e["reach"]
        if c["name"] == "near" and c["groups"] == _lib.GROUP_ALL:
            assert (dmin < 0).mean() >= 0.1 and (dmin > 0).mean() >= 0.3, (case_id(c), (dmin < 0).mean(), (dmin > 0).mean())
            close = reach < 1.0
            assert close.mean() >= 0.2 and (dmin[close] < reach[close]).mean() >= 0.1 and (dmin[close] > reach[close]).mean() >= 0.1, case_id(c)
            near = e["D"] <= dmin + 2 * G
            alone = near.sum(0) == 1
            owner = e["segs"][near.argmax(0)]
            # (several primitives of one seg -- hand spheres and link 6, the object's spheres -- are one seg: unique means one SEG in N)
            for j in np.flatnonzero(~alone):
                if len(set(e["segs"][near[:, j]])) == 1:
                    alone[j] = True
            counts = unique.setdefault((c["task"], c["obj"]), {})
            for s in owner[alone]:
                counts[s] = counts.get(s, 0) + 1
        if c["name"] == "hole" and c["groups"] == _lib.GROUP_HOLE:
            hl, rin, rout = R._tube(0.0)
            ax, rho = _tube_coords(e["p"])
            assert (dmin < 0).mean() >= 0.1 and ((rho < rin) & (np.abs(ax) <= hl)).mean() >= 0.25 and (np.abs(ax) > hl).mean() >= 0.1, case_id(c)
        if c["name"] == "inside" and c["task"] == "peg" and c["groups"] in (_lib.GROUP_FINGERS, _lib.GROUP_HOLE):
            for i, pr in enumerate(e["prims"]):
                rows = slice(N_INSIDE * i, N_INSIDE * (i + 1))
                inside_deep[(pr.seg)] = inside_deep.get(pr.seg, 0) + int((e["D"][i][rows] < -1e-3).sum())
    assert len(unique) == 3
    for (task, obj), counts in unique.items():
        want = [s for s in RY.reachable_segs(task) if not (task == "peg" and s in (1, 5))]
        got = {s: counts.get(s, 0) for s in want}
        assert min(got.values()) >= 3, (task, obj, got)
    assert sorted(inside_deep) == sorted([R.SEG_FINGER0, R.SEG_FINGER0 + 1, _lib.VIEW_SEG_HOLE]) and min(inside_deep.values()) >= 3, inside_deep


def bad_query_block():
    """float32 [8, 4] queries in the env frame and the rows that are bad: NaN and Inf words, a word beyond 1e15, reach 0, a negative reach;
    rows 0, 3 and 7 are one good query, 0.55 above the table in a corner of the workspace that nothing else reaches"""
    good = [-0.5, -0.8, 0.5, 10.0]
    q = np.array([good, [np.nan, 0.2, 0.3, 1.0], [0.3, 0.0, np.inf, 1.0], good, [0.3, 0.0, 0.5, 0.0], [0.3, -3e15, 0.5, 1.0], [0.3, 0.0, 0.5, -1.0], good], dtype=np.float32)
    return q, (1, 2, 4, 5, 6)


def check_bad_queries(out, q, bad):
    """records of the block against the table alone, env-local frame: the bad rows hold the miss record with words 0 and 2 .. 4 as given,
    bit for bit; the good rows name the table"""
    out = np.asarray(out, dtype=np.float32)
    for r in range(len(q)):
        if r in bad:
            assert out[r, 1] == _lib.SEG_NONE and (out[r, 5:] == 0).all(), (r, out[r])
            assert np.array_equal(out[r, [0, 2, 3, 4]], q[r, [3, 0, 1, 2]], equal_nan=True), (r, out[r])
        else:
            assert abs(out[r, 0] - 0.55) < 1e-6 and out[r, 1] in (_lib.SEG_TABLE, _lib.VIEW_SEG_TABLE) and (out[r, 5:] == [0, 0, 1]).all(), (r, out[r])
            assert (out[r] == out[0]).all()


# ------------------------------------------------------------------------------------------------ the measurement behind G_HOST
def measure_host(tmpdir):
    """prints, for the fp32 host build, the failures per grid value of G and the largest use of G"""
    from oracle import oracle as O
    from tests.emul import dist_emul
    cases = make_cases(O)
    L = dist_emul.lib(tmpdir, "f32")
    outs = [dist_emul.closest(L, c) for c in cases]
    exps = [expected(c) for c in cases]
    for G in RY.G_GRID:
        res = [judge(c, G, o, e) for c, o, e in zip(cases, outs, exps)]
        bad = [(case_id(c), r["fail"]) for c, r in zip(cases, res) if r["fail"]]
        worst = max(zip(res, cases), key=lambda rc: rc[0]["use"])
        print("G = %g: %d of %d cases fail %s; largest use of G %.3f (%s); left out at most %.4f; multi-seg share at most %.3f"
              % (G, len(bad), len(cases), bad[:3], worst[0]["use"], case_id(worst[1]), max(r["left_out"] for r in res),
                 max(multi_seg_share(e, G) for c, e in zip(cases, exps) if c["name"] != "degenerate")))


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        measure_host(d)
