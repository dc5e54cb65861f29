"""KDE (package_bgs/ae, BGS_KDE) on the CPU: the numpy restatement (tests/kde_numpy.py) against the masks of the reference's
own code (tests/golden/kde_ref*.npz: pinned), the C ABI defaults and the parameter limits."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

import kde_numpy as kn
from tracking_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["default", "update0", "rgb", "gray", "nosd", "sl8", "th_alpha"]


def golden_cases():
    """{case: (record, input frames)} of every fixture; the input of each is checked against the CRC-32 it was made from."""
    z = np.load(os.path.join(GOLDEN, "kde_ref.npz"))
    clips = {"frames_96x80": np.load(os.path.join(GOLDEN, "frames_96x80.npz"))["frames"],
             "frames_gray_64x48": np.load(os.path.join(GOLDEN, "frames_gray_64x48.npz"))["frames"], "long_clip": kn.long_clip()}
    out = {}
    for c in CASES:
        out[c] = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(c + "/")}
    out["long"] = dict(np.load(os.path.join(GOLDEN, "kde_ref_long.npz")))
    res = {}
    for c, r in out.items():
        p = json.loads(str(r["params"]))
        frames = clips[p["input"]]
        assert zlib.crc32(frames.tobytes()) == int(r["input_crc32"]), "%s: input clip differs from the one the fixture was made from" % c
        res[c] = (r, p, frames)
    return res


def masks_of(r):
    rows, cols = int(r["shape"][1]), int(r["shape"][2])
    return np.unpackbits(r["masks"], axis=-1)[..., :cols].reshape(-1, rows, cols) * np.uint8(255)


def kde_kwargs(p):
    return {k: p[k] for k in ("frames_to_learn", "sequence_length", "time_window", "sd_estimation", "color_ratios", "threshold", "alpha", "update_model")}


@pytest.mark.parametrize("case", CASES + ["long"])
def test_restatement_matches_reference_fixture(case):
    r, p, frames = golden_cases()[case]
    k = kn.Kde(**kde_kwargs(p))
    outs = [k.process(f) for f in frames]
    assert all(o is None for o in outs[:p["frames_to_learn"]])
    got = np.array(outs[p["frames_to_learn"]:])
    want = masks_of(r)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    assert not len(bad), "%s: frames %s differ" % (case, bad[:5])
    if case == "long":  # model state of the reference object after the last frame
        for name, v in k.planes().items():
            assert np.array_equal(v, r[name]), name


def test_long_fixture_exercises_suppression_and_relearning():
    """The novel block is foreground for 500 frames, suppressed by AccMask, then relearnt (it stays background)."""
    r, p, frames = golden_cases()["long"]
    m = masks_of(r)[:, 6, 7]
    first = p["frames_to_learn"]
    assert (m[20 - first:20 - first + 500] == 255).all()
    assert (m[-20:] == 0).all()
    assert int(r["acc"].reshape(16, 16)[6, 7]) == 0  # relearnt: background again, so AccMask restarted


def test_kernel_table_rows_are_normalised():
    t = kn.table()
    assert t.shape == (80, 511)
    assert np.array_equal(t[:, 255 + 1:], t[:, :255][:, ::-1])  # symmetric
    assert np.allclose(t.sum(1), 1.0, rtol=0, atol=1e-12) and np.all(t >= 0)


def test_gate_table():
    g = kn.gate_table(0.3)
    assert tuple(g[0]) == (-3, 3) and tuple(g[9]) == (6, 12)  # g < 3 / alpha: g -/+ 3
    assert tuple(g[10]) == (7, 13) and tuple(g[255]) == (179, 332)  # (int)(g * 0.7 + 0.5), (int)(g * 1.3 + 0.5)
    assert tuple(kn.gate_table(0.5)[255]) == (155, 355)  # g > 100 / alpha: g -/+ 100


def test_bgr2sngnrn_spot_values():
    px = np.array([[0, 0, 0], [255, 255, 255], [0, 255, 0], [10, 20, 30]], np.uint8)  # s = 255 / (b+g+r+30): 265 * 255 / 285 = 237.1
    out = kn.bgr2sngnrn(px)
    assert out.tolist() == [[0, 85, 85], [255, 85, 85], [85, 237, 8], [20, 85, 113]]


def test_default_params_hold_the_reference_defaults():
    p = capi.default_params(capi.KDE)
    assert capi.KDE == 18
    assert (p.kde_frames_to_learn, p.kde_sequence_length, p.kde_time_window) == (10, 50, 100)  # KDE.cpp:19-20
    assert (p.kde_sd_estimation, p.kde_color_ratios, p.kde_update_model) == (1, 1, 1)
    assert p.kde_threshold == 10e-8 and p.kde_alpha == 0.3
    for algo in range(18):  # the kde_* fields stay zero for every other algorithm
        q = capi.default_params(algo)
        assert (q.kde_frames_to_learn, q.kde_sequence_length, q.kde_threshold, q.kde_alpha) == (0, 0, 0.0, 0.0), algo
    assert capi.lib().bgs_abi_version() == 1


def test_params_struct_tail_matches_c(tmp_path):
    import subprocess
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src = tmp_path / "kde_sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%zu %zu %zu %d\\n", sizeof(bgs_params), '
                   'offsetof(bgs_params, kde_frames_to_learn), offsetof(bgs_params, kde_alpha), (int)BGS_KDE);return 0;}\n')
    exe = tmp_path / "kde_sz"
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    size, a, b, k = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(capi.BgsParams) and k == capi.KDE
    assert a == capi.BgsParams.kde_frames_to_learn.offset and b == capi.BgsParams.kde_alpha.offset


@pytest.mark.parametrize("field,value", [("kde_sequence_length", 2), ("kde_sequence_length", 256), ("kde_sequence_length", 0),
                                         ("kde_frames_to_learn", 0), ("kde_time_window", 0), ("kde_time_window", 3 * 256)])
def test_parameter_limits_are_rejected(field, value):
    p = capi.default_params(capi.KDE)
    setattr(p, field, value)
    if field == "kde_time_window" and value > 1:
        p.kde_sequence_length = 3  # 768 / 3 = 256 temporal frames: more than the reference's byte holds
    h = C.c_void_p()
    assert capi.lib().bgs_create(capi.KDE, C.byref(p), 0, 1, C.byref(h)) == capi.ERR_INVALID
    assert b"KDE" in capi.lib().bgs_last_error()
