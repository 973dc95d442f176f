"""The table of bad (and a few good) camera calls that tools/record_render_errors.py records into tests/golden/render_errors.json and
tests/test_gpu_render_errors.py replays against it: one Python list, built by table(), and run_case(), the one way a row is turned into a call.
A row is (entry point, task of the handle, case name, arguments); an argument left out has the value of DEFAULTS."""
import ctypes as C

from peg_in_hole_gym_amd import _lib
from tests.render_cases import BAD_LIGHTS, DEGENERATE, camera_with

N, W, H = 3, 16, 8          # envs per handle, image size
SHADED, EE, RGBA8, DEPTH, CAM_DEV, EE_POS, LIGHT_DEV = (_lib.RENDER_SHADED, _lib.RENDER_CAM_EE, _lib.RENDER_OUT_RGBA8, _lib.RENDER_OUT_DEPTH,
                                                        _lib.RENDER_CAM_DEVICE, _lib.RENDER_CAM_EE_POS, _lib.RENDER_LIGHT_DEVICE)
UNKNOWN = 128               # a bit no entry point knows
# out: "ok" | "null" | "misaligned" (4 bytes past a 16-byte boundary); cam / light: None (NULL), a list of words (host), "device" (a [N, words]
# device array of the task's preset)
DEFAULTS = dict(out="ok", width=W, height=H, env_begin=0, env_count=N, flags=0, cam=None, light=None)
# entry point -> (task of its handle, has flags, has a camera, has a light); pih_render_lit serves both tasks
ENTRIES = (("pih_render", "peg", False, False, False), ("pih_render_ex", "peg", True, False, False), ("pih_render_cam", "fly", True, True, False),
           ("pih_render_view", "peg", True, True, False), ("pih_render_lit", "peg", True, True, True), ("pih_render_lit", "fly", True, True, True))


def table():
    rows = []
    for entry, task, has_flags, has_cam, has_light in ENTRIES:
        other = "fly" if task == "peg" else "peg"
        add = lambda name, on=task, **a: rows.append((entry, on, name, a))
        degenerate = camera_with(**DEGENERATE[0][0])
        add("good call")
        add("NULL out", out="null")
        add("width 0", width=0)
        add("height 0", height=0)
        add("env_begin + env_count past the end", env_begin=1)
        add("env_begin negative", env_begin=-1, env_count=1)
        add("env_count 0", env_count=0)
        add("out misaligned by 4 bytes", out="misaligned")
        if not (has_cam and has_light):          # (pih_render_lit takes the handle of either task)
            add("handle of the wrong task", on=other)
            add("double fault: wrong task + width 0", on=other, width=0)
        if not has_flags:
            continue
        add("good call, shaded", flags=SHADED)
        for bit in (EE, RGBA8, DEPTH, CAM_DEV, EE_POS, LIGHT_DEV, UNKNOWN):
            # (a bit the entry point knows gives a good call here, or the NULL-array message of the two device flags)
            add("flag bit %d alone, NULL camera and light" % bit, flags=bit)
        add("both output formats", flags=RGBA8 | DEPTH)
        add("CAM_EE with CAM_EE_POS", flags=EE | EE_POS)
        add("double fault: unknown flag + misaligned out", flags=UNKNOWN, out="misaligned")
        if not has_cam:
            continue
        add("good call, device cameras, rgba8", flags=CAM_DEV | RGBA8, cam="device")
        add("double fault: both formats + degenerate camera", flags=RGBA8 | DEPTH, cam=degenerate)
        for kw, _ in DEGENERATE:
            add("degenerate camera: %s" % ", ".join("%s=%r" % kv for kv in sorted(kw.items())), cam=camera_with(**kw))
        for i in range(_lib.CAM_WORDS):
            for v in ("nan", "inf"):
                cam = list(_lib.FLY_CAM_DEFAULT); cam[i] = float(v)
                add("camera word %d is %s" % (i, v), cam=cam)
        if not has_light:
            continue
        add("good call, device lights, depth", flags=LIGHT_DEV | DEPTH, light="device")
        add("LIGHT_DEVICE with a NULL light, device cameras", flags=LIGHT_DEV | CAM_DEV, cam="device")
        for k, (field, _, words) in enumerate(BAD_LIGHTS):
            add("degenerate light %d: %s" % (k, field), light=list(words))
        add("double fault: degenerate camera + degenerate light", cam=degenerate, light=list(BAD_LIGHTS[0][2]))
    return rows


class Handles:
    """the two 3-env handles, and for each an output buffer and device arrays of its preset camera and the default light"""

    def __init__(self, torch, peg, fly):
        self.torch, self.g = torch, {"peg": peg, "fly": fly}
        self.out, self.cams, self.lights = {}, {}, {}
        for task, g in self.g.items():
            assert g.n == N
            self.out[task] = torch.zeros(N * H * W * 4 + 8, dtype=torch.float32, device=g.device)
            assert self.out[task].data_ptr() % 16 == 0
            self.cams[task] = torch.tensor([_lib.VIEW_CAM_WRIST if task == "peg" else _lib.FLY_CAM_DEFAULT] * N, dtype=torch.float32, device=g.device)
            self.lights[task] = torch.tensor([_lib.LIGHT_DEFAULT] * N, dtype=torch.float32, device=g.device)


def run_case(hs, row):
    """-> (return code, pih_last_error text after the call)"""
    entry, task, _, given = row
    a = dict(DEFAULTS, **given)
    g = hs.g[task]
    out = {"ok": hs.out[task].data_ptr(), "null": None, "misaligned": hs.out[task].data_ptr() + 4}[a["out"]]

    def words(v, dev, count):
        if v is None:
            return None
        return dev[task].data_ptr() if v == "device" else (C.c_float * count)(*v)

    cam, light = words(a["cam"], hs.cams, _lib.CAM_WORDS), words(a["light"], hs.lights, _lib.LIGHT_WORDS)
    size = (a["width"], a["height"], a["env_begin"], a["env_count"])
    f = getattr(g.L, entry)
    if entry == "pih_render":
        code = f(g.h, out, *size, None)
    elif entry == "pih_render_ex":
        code = f(g.h, out, *size, a["flags"], None)
    elif entry == "pih_render_lit":
        code = f(g.h, out, cam, light, *size, a["flags"], None)
    else:
        code = f(g.h, out, cam, *size, a["flags"], None)
    hs.torch.cuda.synchronize()
    return code, g.L.pih_last_error(g.h).decode()


def run_table(hs):
    """-> the rows of the golden file: [entry point, "task: case name", return code, text]"""
    return [[row[0], "%s handle: %s" % (row[1], row[2]), *run_case(hs, row)] for row in table()]
