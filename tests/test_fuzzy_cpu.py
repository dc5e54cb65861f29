"""FuzzySugenoIntegral / FuzzyChoquetIntegral (BGS_FUZZY_SUGENO / BGS_FUZZY_CHOQUET, USTC_BGS types 21 and 22) without a GPU: the numpy
restatement against the reference's own FuzzyUtils / PixelUtils (tests/golden/fuzzy_ref.npz), what each fixture case covers, the C
ABI (ids, the second hole, bgs_fuzzy_params, every refusal) and the host layer."""
import ctypes as C
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import fuzzy_numpy as fz
from tracking_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
REF = np.load(os.path.join(GOLDEN, "fuzzy_ref.npz"))
CASES = ["choquet_default", "sugeno_default", "choquet_opt1", "sugeno_opt1", "nosmooth", "portrait", "square", "tiny3x3", "tiny2x2", "thr_edge", "relearn", "flat"]
SIZEOF_BGS_PARAMS_PARENT = 336  # sizeof(bgs_params) of the commit before this class: bgs_params must not grow


def golden(case):
    """(fixture entries, per-frame parameter dicts, frames) of a case; the frames are crops of the committed clip (or zeros)."""
    r = {k.split("/", 1)[1]: REF[k] for k in REF.files if k.startswith(case + "/")}
    c = json.loads(str(r["crop"]))
    if c.get("zero"):
        frames = np.zeros((c["T"], c["h"], c["w"], 3), np.uint8)
    else:
        clip = np.load(os.path.join(GOLDEN, "frames_96x80.npz"))["frames"]
        frames = np.ascontiguousarray(clip[c["t0"]:c["t0"] + c["T"], c["y0"]:c["y0"] + c["h"], c["x0"]:c["x0"] + c["w"]])
    assert zlib.crc32(frames.tobytes()) == int(r["input_crc32"])
    return r, json.loads(str(r["params"])), frames


def masks_of(r, W):
    return np.unpackbits(r["masks"], axis=-1, bitorder="little")[..., :W] * np.uint8(255)


def same_floats(got, bits):
    """Equal bit for bit where the fixture holds a number, NaN where it holds a NaN."""
    want = bits.view(np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], bits[~nan])


def check_against_fixture(case, step, state):
    """Runs a case frame by frame through step(frame, params) -> (mask or None, background bytes or None) and compares everything the
    fixture holds; state() -> (float background (H,W,3), integral (H,W)) at the end."""
    r, plist, frames = golden(case)
    W = frames.shape[2]
    want = masks_of(r, W)
    defined = int(r["masks_defined"]) if "masks_defined" in r else len(want)
    k = 0
    for t, f in enumerate(frames):
        mask, bgu = step(f, plist[t])
        assert (mask is not None) == bool(r["valid"][t]) == (bgu is not None), (case, t)
        if mask is None:
            continue
        if k < defined:
            assert np.array_equal(mask, want[k]), (case, t, int((mask != want[k]).sum()))
        else:  # the reference reads uninitialised heap here: the defined behaviour is NaN -> every pixel foreground
            assert (mask == 255).all(), (case, t)
        assert zlib.crc32(np.ascontiguousarray(bgu).tobytes()) == int(r["bg_crc32"][t]), (case, t)
        k += 1
    assert k == len(want) and np.array_equal(bgu, r["bg_last"])
    if "bgf_bits" in r:
        bg, integral = state()
        assert same_floats(bg, r["bgf_bits"]), case
        if defined == len(want):
            assert same_floats(integral, r["integral_bits"]), case


def run_restatement(case, **kw):
    """The restatement over a case, compared with the fixture (not with `identity_indice`, which is not the reference); returns it."""
    r, plist, frames = golden(case)
    m = fz.Fuzzy(int(r["kind"]), **kw)
    if kw:
        for f, p in zip(frames, plist):
            m.process(f, **p)
    else:
        check_against_fixture(case, lambda f, p: m.process(f, **p), lambda: (m.bg, m.integral))
    return m


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_fixture(case):
    run_restatement(case)


def test_fixture_file_is_small_and_complete():
    assert os.path.getsize(os.path.join(GOLDEN, "fuzzy_ref.npz")) <= 122 * 1024
    assert sorted({k.split("/")[0] for k in REF.files}) == sorted(CASES)


@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith("tiny") and c != "flat"])
def test_both_mask_values_occur(case):
    r, _, frames = golden(case)
    m = masks_of(r, frames.shape[2])
    assert (m == 0).any() and (m == 255).any()


def test_landscape_lbp_column_h_repeats_column_h_minus_1_and_portrait_row_w_is_its_own_formula():
    m = run_restatement("choquet_default")
    H, W = m.lbp_in.shape
    assert W >= H + 2
    for img in (m.lbp_in, m.lbp_bg):
        assert np.array_equal(img[1:-1, H], img[1:-1, H - 1]) and img[1:-1, H - 1].any()
    _, _, frames = golden("choquet_default")
    plain = fz.lbp_plain(fz.gray(frames[-1].astype(np.float32) * np.float32(1 / 255.)))
    assert not np.array_equal(plain[1:-1, H], m.lbp_in[1:-1, H]) and np.array_equal(np.delete(plain, H, 1)[1:-1], np.delete(m.lbp_in, H, 1)[1:-1])
    p = run_restatement("portrait")
    H, W = p.lbp_in.shape
    assert H >= W + 2
    _, _, frames = golden("portrait")
    plain = fz.lbp_plain(fz.gray(frames[-1].astype(np.float32) * np.float32(1 / 255.)))
    assert not np.array_equal(plain[W, 1:-1], p.lbp_in[W, 1:-1]) and np.array_equal(np.delete(plain, W, 0)[1:], np.delete(p.lbp_in, W, 0)[1:])
    sq = run_restatement("square")
    _, _, frames = golden("square")
    plain = fz.lbp_plain(fz.gray(frames[-1].astype(np.float32) * np.float32(1 / 255.)))
    plain[0, 0] = sq.lbp_in[0, 0]
    assert np.array_equal(plain, sq.lbp_in)  # square frames hit neither branch
    assert (sq.lbp_in[0, 1:] == 0).all() and (sq.lbp_in[-1] == 0).all() and (sq.lbp_in[1:, 0] == 0).all() and (sq.lbp_in[:, -1] == 0).all()


@pytest.mark.parametrize("case", ["choquet_default", "sugeno_default"])
def test_the_integral_depends_on_raster_order(case):
    """Some pixel's value differs from what a per-pixel Indice = (0,1,2) would give, so the fixture pins the prefix over the frame."""
    a, b = run_restatement(case), run_restatement(case, identity_indice=True)
    assert (a.integral != b.integral).sum() > 10


def test_prefix_product_equals_the_serial_loop():
    rng = np.random.default_rng(3)
    pi = np.stack([rng.permutation(3) for _ in range(1000)])
    idx, want = np.arange(3), []
    for p in pi:
        idx = idx[p]
        want.append(idx)
    assert np.array_equal(fz.prefix_perm(pi), np.stack(want))


def test_flat_goes_nan():
    m = run_restatement("flat")
    assert np.isnan(m.bg).all() and np.isnan(REF["flat/bgf_bits"].view(np.float32)).all()
    assert (REF["flat/bg_last"] == 0).all()  # NaN -> 0 in the byte image


def test_threshold_case_flips_masks_both_ways():
    r, _, frames = golden("thr_edge")
    m = masks_of(r, frames.shape[2]).astype(int)
    assert (((m[1:] > m[:-1]).any(0)) & ((m[1:] < m[:-1]).any(0))).any()


def test_relearn_goes_back_to_learning():
    r, plist, _ = golden("relearn")
    v = r["valid"].tolist()
    assert plist[0]["ftl"] < plist[-1]["ftl"] and v[:3] == [0, 0, 0] and 1 in v[3:6] and v[6:9] == [0, 0, 0] and v[-1] == 1


def test_lbp_table_equals_the_stepwise_sum():
    tab = fz.lbp_table()
    w = [1, 2, 4, 8, 16, 32, 64, 128]
    assert len(set(tab.tolist())) == 256 and tab[0] == 0
    for code in (0, 1, 37, 128, 200, 255):
        v = np.float32(0)
        for l in range(9):  # nine steps, the centre's term is 1 * 0 / 255
            term = 0.0 if l == 4 else float(((code >> (l if l < 4 else l - 1)) & 1) * w[l if l < 4 else l - 1]) / 255.0
            v = np.float32(float(v) + term)
        assert tab[code] == v


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

FZ_FIELDS = ["struct_size", "frames_to_learn", "alpha_learn", "alpha_update", "color_space", "option", "smooth", "threshold"]


def test_ids_holes_and_struct_layout_match_c(tmp_path):
    inc = os.path.join(HERE, os.pardir, "include")
    src = tmp_path / "fz_abi.c"
    ids = (-1, 0, 25, 26, 27, 28, 29, 30, 31, 99)
    known = ", ".join("BGS_ALGO_KNOWN(%d)" % i for i in ids)
    offs = ", ".join("offsetof(bgs_fuzzy_params, %s)" % f for f in FZ_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%zu %zu %d %d %d' + " %d" * len(ids) + " %zu" * len(FZ_FIELDS)
                   + '\\n", sizeof(bgs_params), sizeof(bgs_fuzzy_params), (int)BGS_ALGO_LIMIT, (int)BGS_FUZZY_SUGENO, (int)BGS_FUZZY_CHOQUET, ' + known + ", " + offs + ");return 0;}\n")
    exe = tmp_path / "fz_abi"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert v[0] == SIZEOF_BGS_PARAMS_PARENT == C.sizeof(capi.BgsParams)
    assert v[1] == C.sizeof(capi.BgsFuzzyParams) == 48
    assert v[2:5] == [28, 29, 30] and (capi.ALGO_LIMIT, capi.FUZZY_SUGENO, capi.FUZZY_CHOQUET) == (28, 29, 30)
    assert v[5:5 + len(ids)] == [0, 1, 1, 0, 1, 0, 1, 1, 0, 0]
    assert v[5 + len(ids):] == [getattr(capi.BgsFuzzyParams, f).offset for f in FZ_FIELDS] == [0, 4, 8, 16, 24, 28, 32, 40]


def test_unknown_ids_stay_unknown_and_range_checks_use_the_one_helper():
    p = capi.BgsParams()
    p.struct_size = C.sizeof(capi.BgsParams)
    for bad in (26, 28, 31, 99, -1):
        assert capi.lib().bgs_default_params(bad, C.byref(p)) == capi.ERR_INVALID, bad
        h = C.c_void_p()
        assert capi.lib().bgs_create(bad, None, 0, 1, C.byref(h)) == capi.ERR_INVALID and b"unknown algorithm" in capi.lib().bgs_last_error()
    for ok in (29, 30):
        assert capi.lib().bgs_default_params(ok, C.byref(p)) == capi.OK
    for src in ("bgs_hip.hip", "bgs_node.cpp"):
        text = open(os.path.join(HERE, os.pardir, "tracking_amd", "csrc", src)).read()
        assert "BGS_ALGO_KNOWN(algo)" in text and ">= BGS_ALGO_LIMIT" not in text and ">= BGS_ALGO_LAST" not in text, src


def test_default_fuzzy_params():
    p = capi.fuzzy_default_params()
    assert (p.struct_size, p.frames_to_learn, p.alpha_learn, p.alpha_update, p.color_space, p.option, p.smooth, p.threshold) == (48, 10, 0.1, 0.01, 1, 2, 1, 0.67)
    d = fz.DEFAULTS
    assert (p.frames_to_learn, p.alpha_learn, p.alpha_update, p.option, p.smooth, p.threshold) == (d["ftl"], d["alphaLearn"], d["alphaUpdate"], d["option"], d["smooth"], d["threshold"])
    assert capi.lib().bgs_fuzzy_default_params(None) == capi.ERR_INVALID


@pytest.mark.parametrize("algo,name", [(capi.FUZZY_SUGENO, b"FuzzySugenoIntegral"), (capi.FUZZY_CHOQUET, b"FuzzyChoquetIntegral")])
def test_every_refusal_names_the_class_and_needs_no_device(algo, name):
    check = capi.lib().bgs_fuzzy_check
    assert check(algo, None, 0, 0, 0) == capi.OK and check(algo, None, 80, 96, 3) == capi.OK and check(algo, None, 2, 2, 3) == capi.OK
    for kw in (dict(color_space=2), dict(color_space=3), dict(color_space=4), dict(option=0), dict(option=3)):
        p = capi.fuzzy_default_params(**kw)
        assert check(algo, C.byref(p), 0, 0, 0) == capi.ERR_UNSUPPORTED, kw
        assert name in capi.lib().bgs_last_error(), kw
    assert check(algo, C.byref(capi.fuzzy_default_params(color_space=2)), 0, 0, 0) == capi.ERR_UNSUPPORTED and b"Ohta" in capi.lib().bgs_last_error()
    for rows, cols, ch in ((80, 96, 1), (1, 96, 3), (80, 1, 3)):
        assert check(algo, None, rows, cols, ch) == capi.ERR_UNSUPPORTED, (rows, cols, ch)
        assert name in capi.lib().bgs_last_error()
    assert check(algo, C.byref(capi.fuzzy_default_params(frames_to_learn=-1)), 0, 0, 0) == capi.ERR_INVALID
    assert check(algo, C.byref(capi.fuzzy_default_params(struct_size=40)), 0, 0, 0) == capi.ERR_INVALID
    assert check(capi.VUMETER, None, 0, 0, 0) == capi.ERR_INVALID
    m = fz.Fuzzy(fz.CHOQUET, ftl=0, option=3)  # the restatement refuses it too, on the first detecting frame
    m.process(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        m.process(np.zeros((4, 4, 3), np.uint8))


def test_ohta_finding():
    """Why colorSpace 2 is refused: I2 = (R - B) / 2 is 0 for R == B; against a negative I2 the ratio `bg / cur` is -x / 0 = -inf."""
    with np.errstate(all="ignore"):
        cur, bg = np.float32(0.0), np.float32(-0.05)  # current I2 (R == B) and a background I2 with R < B
        assert cur > bg and bg / cur == -np.inf


# ---- host layer ------------------------------------------------------------------------------------------------------------------------

def test_reference_side_adapters_compile_with_the_fuzzy_classes(tmp_path):
    root = os.path.dirname(HERE)
    tu = tmp_path / "adapters_fz.cpp"
    tu.write_text('#include "HipBGS.h"\n#include "HipFGDetector.h"\nIBGS* a() { return new hipbgs::FuzzySugenoIntegral; }\nIBGS* b() { return new hipbgs::FuzzyChoquetIntegral; }\n'
                  "CvFGDetector* c() { return new HipFGDetector(21); }\nCvFGDetector* d() { return new HipFGDetector(22); }\n")
    r = subprocess.run(["g++", "-std=gnu++0x", "-fsyntax-only", "-Wall", "-I" + os.path.join(root, "tests", "mock_opencv"), "-I" + os.path.join(root, "include"),
                        "-I" + os.path.join(root, "tracking_amd", "host"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
