"""The five package_bgs/lb/ models (BGS_LB_*, USTC_BGS types 25-29) on the CPU: the numpy restatement (tests/lb_numpy.py) against
the outputs of the reference's own code (tests/golden/lb_ref_*.npz: pinned), the measurement behind the fuzzy classes' plane
tolerance, what the fixtures claim to cover, the C ABI (ids, struct tail, defaults, refusals) and the host class list."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import lb_numpy as ln
from tracking_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SHORT = {25: "sg", 26: "fg", 27: "mog", 28: "som", 29: "fsom"}
CLASSES = [25, 26, 27, 28, 29]
EXACT, FUZZY = (25, 27, 28), (26, 29)
CASES = ["default", "params", "modes", "ties_fast", "long", "change"]
WHOLE_MODEL = ["modes", "ties_fast", "long"]  # the cases that hold every model plane after the last frame
ALGO = {25: "LB_SIMPLE_GAUSSIAN", 26: "LB_FUZZY_GAUSSIAN", 27: "LB_MOG", 28: "LB_ADAPTIVE_SOM", 29: "LB_FUZZY_ADAPTIVE_SOM"}
LB_FIELDS = ["lb_sensitivity", "lb_bg_threshold", "lb_learning_rate", "lb_noise_variance", "lb_training_sensitivity",
             "lb_training_learning_rate", "lb_training_steps"]


def _clip(name):
    if name == "frames_96x80":
        return np.load(os.path.join(GOLDEN, "frames_96x80.npz"))["frames"]
    kind, T, H, W, seed = name.split(":")
    return getattr(ln, kind)(int(T), int(H), int(W), int(seed))


def golden(cls, case):
    """(record, keyword parameters, (frame, changed parameters) or None, input frames) of one fixture case; the input is checked
    against the CRC-32 it was made from."""
    z = np.load(os.path.join(GOLDEN, "lb_ref_%s.npz" % SHORT[cls]))
    r = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(case + "/")}
    p = json.loads(str(r["params"]))
    frames = _clip(p.pop("input"))
    change = p.pop("change", None)
    assert ln.crc(frames) == int(r["input_crc32"]), "%s: input clip differs from the one the fixture was made from" % case
    return r, p, change, frames


def masks_of(r):
    T, rows, cols = (int(v) for v in r["shape"])
    return np.unpackbits(r["masks"], axis=-1)[..., :cols].reshape(T, rows, cols) * np.uint8(255)


def run_restatement(cls, case, exp=None):
    """-> (model, mask bits that differ, background frames whose CRC differs, last background equal, record)"""
    r, p, change, frames = golden(cls, case)
    m = ln.LB(cls, exp=exp, **p)
    want = masks_of(r)
    bad_bits = bad_bg = 0
    for t, f in enumerate(frames):
        if change and t == change[0]:
            m.set(**change[1])
        fg, bg = m.process(f)
        bad_bits += int((fg != want[t]).sum())
        bad_bg += int(ln.crc(bg) != int(r["bg_crc32"][t]))
    return m, bad_bits, bad_bg, np.array_equal(bg, r["bg_last"]), r


def plane_deviation(m, r):
    return {k: float(np.abs(v.astype(np.float64) - r[k].astype(np.float64).reshape(v.shape)).max()) for k, v in m.planes().items() if k in r}


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cls", EXACT)
def test_restatement_equals_reference_fixture_bit_for_bit(cls, case):
    m, bad_bits, bad_bg, last_ok, r = run_restatement(cls, case)
    assert (bad_bits, bad_bg, last_ok) == (0, 0, True)
    if case in WHOLE_MODEL:
        planes = m.planes()
        assert set(planes) <= set(r), set(planes) - set(r)
        for name, v in planes.items():
            assert np.array_equal(v, r[name].reshape(v.shape)), name


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cls", FUZZY)
def test_fuzzy_restatement_against_reference_fixture(cls, case):
    """Masks and background bytes exactly; the planes exactly where this machine's libm exp() reproduces the fixture's (same glibc
    family), else within the tolerance of lb_numpy.FUZZY_PLANE_TOL - which of the two is detected, nothing is skipped."""
    m, bad_bits, bad_bg, last_ok, r = run_restatement(cls, case)
    assert (bad_bits, bad_bg, last_ok) == (0, 0, True)
    if case in WHOLE_MODEL:
        dev = plane_deviation(m, r)
        assert set(dev) == set(m.planes())
        same_libm = all(v == 0.0 for v in dev.values())
        print("class %d %s: libm exp %s the fixture's planes %s" % (cls, case, "reproduces" if same_libm else "does not reproduce", dev))
        for name, d in dev.items():
            tol = ln.FUZZY_PLANE_TOL[cls].get(name, 0.0)  # "bg", "count": exact
            assert d == 0.0 if same_libm else d <= tol, (name, d, tol)


@pytest.mark.parametrize("cls", FUZZY)
def test_a_last_bit_of_exp_moves_no_mask_bit_and_the_tolerance_is_current(cls):
    """exp() nudged one ulp up / down on EVERY call, on every fuzzy fixture: no mask bit and no background byte differs from the
    reference (the condition that lets the GPU tests compare them exactly), and D - the largest deviation of a model plane from the
    reference fixture - is what FUZZY_PLANE_TOL was derived from: 4 D <= tolerance <= 40 D."""
    D = {}
    for case in CASES:
        for name, ex in (("up", ln.exp_up), ("down", ln.exp_down)):
            m, bad_bits, bad_bg, last_ok, r = run_restatement(cls, case, exp=ex)
            assert (bad_bits, bad_bg, last_ok) == (0, 0, True), (case, name)
            if case in WHOLE_MODEL:
                for k, d in plane_deviation(m, r).items():
                    D[k] = max(D.get(k, 0.0), d)
    scale = {"mu": 255.0, "som": 255.0, "var": 255.0 ** 2}
    for k, tol in ln.FUZZY_PLANE_TOL[cls].items():
        print("class %d plane %s: D = %.3e (%.2e of full scale), tolerance %.1e = %.1f D" % (cls, k, D[k], D[k] / scale[k], tol, tol / D[k]))
        assert D[k] > 0 and 4 * D[k] <= tol <= 40 * D[k], (k, D[k], tol)
    assert all(D[k] == 0 for k in D if k not in ln.FUZZY_PLANE_TOL[cls]), D  # "bg", "count"


@pytest.mark.parametrize("cls", CLASSES)
def test_fixtures_cover_what_they_claim(cls):
    for case in CASES:
        r, p, change, frames = golden(cls, case)
        assert set(np.unique(masks_of(r))) == {0, 255}, case  # both mask values
    assert len(golden(cls, "long")[3]) >= 150 and golden(cls, "default")[1] == {} and golden(cls, "change")[2] is not None
    assert golden(cls, "ties_fast")[1]["learning_rate"] == 255  # alpha = 1: d*d guards at exact zeros, variances on their clamp
    for case in WHOLE_MODEL:
        m, _, _, _, r = run_restatement(cls, case)
        if cls == 27:
            assert (r["k"] == 3).any() and m.swaps > 0 and m.replaced > 0, case
            assert (r["w"][r["k"] < 3][:, 2] == 0).all()  # slots >= K as the constructor left them
        if cls in (28, 29):
            tsteps = ln.model_params(m.p)["tsteps"]
            assert int(r["count"][0]) == tsteps + 1 < len(golden(cls, case)[3]), case  # crossed from calibration to the online phase
            assert m.bmu_seen == {"corner", "edge", "centre"}, (case, m.bmu_seen)
    if cls == 27:
        m = run_restatement(27, "modes")[0]
        assert m.first_not_best > 0  # the first mode inside the threshold was not the nearest one
    if cls in (28, 29):  # a pixel that is foreground keeps the byte triple of the last frame it was background
        r, p, change, frames = golden(cls, "modes")
        m = ln.LB(cls, **p)
        stale = 0
        prev = None
        for f in frames:
            fg, bg = m.process(f)
            if prev is not None:
                stale += int(((fg != 0)[..., None] & (bg == prev) & (prev != 0)).all(-1).sum())
                assert np.array_equal(bg[fg != 0], prev[fg != 0])
            prev = bg
        assert stale > 50


def test_parameter_mapping_returns_the_training_steps_that_went_in():
    """(int)(255.0 * (value / 255.0)) == value for every value 0..255, in double."""
    for v in range(256):
        assert ln.model_params(dict(ln.DEFAULTS[28], bg_threshold=0, noise_variance=0, training_steps=v))["tsteps"] == v
    assert 254 / 255.0 < 1 - 2.0 ** -50  # MoG bgThreshold 254: the normalised weights (sum 1 within rounding) always pass m_T


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_ids_and_struct_tail_match_c(tmp_path):
    inc = os.path.join(HERE, os.pardir, "include")
    src = tmp_path / "lb_sz.c"
    fields = ", ".join("offsetof(bgs_params, %s)" % f for f in LB_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%zu %d %d %d %d %d %d %d %zu'
                   + " %zu" * len(LB_FIELDS) + '\\n", sizeof(bgs_params), (int)BGS_ALGO_COUNT, (int)BGS_ALGO_END, (int)BGS_LB_SIMPLE_GAUSSIAN, '
                   '(int)BGS_LB_FUZZY_GAUSSIAN, (int)BGS_LB_MOG, (int)BGS_LB_ADAPTIVE_SOM, (int)BGS_LB_FUZZY_ADAPTIVE_SOM, offsetof(bgs_params, dp_weight), '
                   + fields + ');return 0;}\n')
    exe = tmp_path / "lb_sz"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    size, count, end, ids, dpw, offs = v[0], v[1], v[2], v[3:8], v[8], v[9:]
    assert size == C.sizeof(capi.BgsParams)
    assert count == 21 and end == 26  # the count is frozen, the end marker follows the last id
    assert ids == [getattr(capi, ALGO[c]) for c in CLASSES] == [21, 22, 23, 24, 25]
    assert offs == [getattr(capi.BgsParams, f).offset for f in LB_FIELDS]
    assert offs == sorted(offs) and offs[0] > dpw == capi.BgsParams.dp_weight.offset  # grown at the end only
    assert capi.lib().bgs_abi_version() == 1


def test_default_params_hold_the_wrappers_constructor_values():
    want = {25: (66, 0, 18, 162, 0, 0, 0), 26: (72, 162, 49, 195, 0, 0, 0), 27: (81, 83, 59, 206, 0, 0, 0),
            28: (75, 0, 62, 0, 245, 255, 55), 29: (90, 0, 38, 0, 240, 255, 81)}
    for cls in CLASSES:
        p = capi.default_params(getattr(capi, ALGO[cls]))
        assert tuple(getattr(p, f) for f in LB_FIELDS) == want[cls], cls
        d = dict(ln.DEFAULTS[cls])
        assert all(getattr(p, "lb_" + k) == v for k, v in d.items())
    for algo in range(21):
        q = capi.default_params(algo)
        assert all(getattr(q, f) == 0 for f in LB_FIELDS), algo
    p = capi.BgsParams()
    p.struct_size = C.sizeof(capi.BgsParams)
    for bad in (26, 99, -1):
        assert capi.lib().bgs_default_params(bad, C.byref(p)) == capi.ERR_INVALID
    h = C.c_void_p()
    assert capi.lib().bgs_create(99, None, 0, 1, C.byref(h)) == capi.ERR_INVALID and b"unknown algorithm" in capi.lib().bgs_last_error()


REFUSED = [(c, f, v) for c in CLASSES for f in LB_FIELDS for v in (-1, 256)]
REFUSED += [(25, "lb_noise_variance", 0), (26, "lb_noise_variance", 0), (27, "lb_noise_variance", 0), (27, "lb_bg_threshold", 255),
            (28, "lb_training_steps", 0), (29, "lb_training_steps", 0)]


@pytest.mark.parametrize("cls,field,value", REFUSED)
def test_refused_parameters(cls, field, value):
    """Checked before the GPU is opened: BGS_ERR_UNSUPPORTED with the class name in the message."""
    algo = getattr(capi, ALGO[cls])
    p = capi.default_params(algo)
    setattr(p, field, value)
    h = C.c_void_p()
    assert capi.lib().bgs_create(algo, C.byref(p), 0, 1, C.byref(h)) == capi.ERR_UNSUPPORTED
    assert ln.NAMES[cls].encode() in capi.lib().bgs_last_error()


# ---- host layer ------------------------------------------------------------------------------------------------------------------------

def test_reference_side_adapters_compile_with_the_lb_classes(tmp_path):
    """HipBGS.h / HipFGDetector.h with the five classes, -std=gnu++0x against the declaration-only OpenCV mock (the 8UC3 mask is
    made by hand there: the mock has neither cv::merge nor cv::cvtColor)."""
    root = os.path.dirname(HERE)
    tu = tmp_path / "adapters_lb.cpp"
    tu.write_text('#include "HipBGS.h"\n#include "HipFGDetector.h"\n'
                  'IBGS* make(int i) { if (i == 0) return new hipbgs::LBSimpleGaussian; if (i == 1) return new hipbgs::LBFuzzyGaussian;\n'
                  '  if (i == 2) return new hipbgs::LBMixtureOfGaussians; if (i == 3) return new hipbgs::LBAdaptiveSOM; return new hipbgs::LBFuzzyAdaptiveSOM; }\n'
                  'CvFGDetector* make_fg() { return new HipFGDetector(28); }\n')
    r = subprocess.run(["g++", "-std=gnu++0x", "-fsyntax-only", "-Wall", "-I" + os.path.join(root, "tests", "mock_opencv"), "-I" + os.path.join(root, "include"),
                        "-I" + os.path.join(root, "tracking_amd", "host"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
