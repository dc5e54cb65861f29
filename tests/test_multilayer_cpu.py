"""MultiLayerBGS (USTC_BGS type 23's class) without a GPU: the numpy restatement against the fixture made from the reference's own
jmo/CMultiLayerBGS.cpp, the conditions that make the fixture a fair yardstick (every branch counter above 0, expf mismatch counts 0),
the same restatement against the reference's code on every run of the fixed slices of the models fuzz
(tests/golden/multilayer_fuzz_ref.npz), the C ABI (ids, bgs_multilayer_params, the refusals, the host-computed constants) and the host layer."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import multilayer_numpy as ml
from tracking_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "tracking_amd", "host")
PARAMS = getattr(capi, "BgsMultilayerParams", None)
FIELDS = [f for f, _ in PARAMS._fields_] if PARAMS else []


@functools.lru_cache(maxsize=None)
def restated(case):
    r = ml.load()[case]
    m, masks, bgs = ml.run(r["params"], r["frames"], int(r["consts"][0]))
    return m, masks, bgs


# ---- the restatement and the fixture -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ml.cases())
def test_restatement_reproduces_the_reference_fixture(case):
    r = ml.load()[case]
    m, masks, bgs = restated(case)
    assert np.array_equal(masks, r["masks"])
    assert [ml.crc(b) for b in bgs] == [int(c) for c in r["bg_crc"]]
    order, modes, dist = m.state()
    assert order.tobytes() == r["order"].tobytes()
    assert ml.crc(modes) == r["modes_crc"]
    if "modes" in r:
        assert modes.tobytes() == r["modes"].tobytes()
    assert dist.tobytes() == r["dist"].tobytes()
    assert not r["masks"][0].any()  # a stream's first frame: the zero mask


def _fuzz_slices():
    import model_refs as mr
    return [s for s in mr.SLICES if s[1] == (ml.CLASS_NAME,)]


@pytest.mark.parametrize("classes,big,first,count", [s[1:] for s in _fuzz_slices()], ids=[s[0] for s in _fuzz_slices()])
def test_restatement_reproduces_the_reference_where_the_fuzz_takes_it(classes, big, first, count):
    """tests/golden/multilayer_fuzz_ref.npz: the reference's own code on every stream of every accepted case of the fixed slices of the
    models fuzz, run straight through with the case's parameters (tools/ref_fixtures/multilayer/make_fixture.py), as CRCs of the
    input, the masks, the backgrounds and the three state planes after the last frame."""
    import model_refs as mr
    z = np.load(os.path.join(HERE, "golden", "multilayer_fuzz_ref.npz"))
    rec = {(int(seed), int(s)): [int(c) for c in crcs] for (seed, s), crcs in zip(z["runs"], z["crcs"])}
    assert len(rec) == len(z["runs"]) and (z["expf"][:, 0] > 0).all()
    ad = mr.BY_CLASS[ml.CLASS_NAME]
    bits = int(ml.load()["defaults"]["consts"][0])
    ran = 0
    for case in mr.slice_cases(first, count, classes, big):
        if ad.refusal(ml.CLASS_NAME, case["params"]) is not None:
            assert not any(seed == case["seed"] for seed, _ in rec)
            continue
        for s, frames in enumerate(mr.build_inputs(case)):
            want = rec[case["seed"], s]
            assert ml.crc(frames) == want[0], (case["seed"], s, "the input")
            m, masks, bgs = ml.run(case["params"], frames, bits)
            got = [ml.crc(masks), ml.crc(bgs)] + [ml.crc(a) for a in m.state()]
            assert got == want[1:], (case["seed"], s, "masks, backgrounds, order, modes, dist", [a == b for a, b in zip(got, want[1:])], case["params"])
            ran += 1
    assert ran >= count // 2
    if (big, first) == (False, 715000):  # the file holds the runs of the three slices and nothing else
        runs = sum(c["S"] for sl in _fuzz_slices() for c in mr.slice_cases(sl[3], sl[4], sl[1], sl[2]) if ad.refusal(ml.CLASS_NAME, c["params"]) is None)
        assert runs == len(rec)


def test_a_frame_that_empties_the_last_pixel_s_list_is_a_first_frame_again():
    """weight_updating_constant 5 with a fast weight rate drives a layered mode's weight below zero, the
    first form of the layer removal takes the list's only mode, and when the last pixel is among those pixels the frame gets the
    zero mask in the middle of a stream.  Run (715035, stream 0) of the fuzz fixture is such a clip: the masks are the reference's."""
    import model_refs as mr
    case = mr.slice_cases(715035, 1, (ml.CLASS_NAME,), False)[0]
    assert case["params"]["weight_updating_constant"] == 5.0 and not any(st["resets"] for st in case["steps"])
    m, masks, _ = ml.run(case["params"], mr.build_inputs(case)[0], int(ml.load()["defaults"]["consts"][0]))
    assert masks[3].any() and not masks[4].any() and masks[5].any()
    z = np.load(os.path.join(HERE, "golden", "multilayer_fuzz_ref.npz"))
    i = [tuple(r) for r in z["runs"].tolist()].index((715035, 0))
    assert ml.crc(masks) == int(z["crcs"][i][1])


def test_the_fixture_holds_the_cases_the_class_needs():
    want = {"defaults", "fast", "K1", "K3", "detect_after", "detect_after_nolearn", "status_detect", "no_texture", "no_smooth", "h0", "dark",
            "fast_3x3", "fast_5x7", "fast_9x4", "fast_130x5", "fast_5x130", "fast_65x131"}
    assert want <= set(ml.cases())
    f = ml.load()
    assert f["defaults"]["masks"].shape == (24, 37, 53) and f["fast"]["masks"].shape == (40, 37, 53)
    assert f["K1"]["params"]["max_mode_num"] == 1 and f["K3"]["params"]["max_mode_num"] == 3
    assert f["no_smooth"]["params"]["pattern_neig_half_size"] == -1 and f["h0"]["params"]["pattern_neig_half_size"] == 0
    assert f["no_texture"]["params"]["texture_weight"] == 0 and f["status_detect"]["params"]["status"] == 1
    assert f["detect_after"]["params"]["detect_after"] == 8 and f["detect_after_nolearn"]["params"]["disable_learning"] == 1
    assert all(r["masks"].any() for r in f.values())  # every case detects something
    # the two detect_after cases part at the switch: the model stops learning in one of them
    assert np.array_equal(f["detect_after"]["masks"][:9], f["detect_after_nolearn"]["masks"][:9])
    assert f["detect_after"]["order"].tobytes() != f["detect_after_nolearn"]["order"].tobytes()


def test_every_branch_counter_is_above_zero_somewhere_in_the_fixture():
    total = dict.fromkeys(ml.COUNTERS, 0)
    for case in ml.cases():
        for k, v in restated(case)[0].counts.items():
            total[k] += v
    assert all(v > 0 for v in total.values()), total
    fast = restated("fast")[0]
    assert fast.counts["removal_first"] > 0 and fast.counts["removal_second"] > 0 and fast.counts["replace"] > 0
    assert (fast.state()[1][:, :, 17] == 2).any() or restated("dark")[0].counts["layer_created"] > 0
    assert restated("defaults")[0].counts["layer_created"] > 0


def test_expf_mismatch_counts_are_zero():
    for case, r in ml.load().items():
        assert int(r["expf"][1]) == 0 and int(r["expf"][0]) > 0, case


def test_quicksort_tie_order_is_the_reference_s():
    """equal weights swap their indices: the literal sort is not a stable sort"""
    d, p = [0.5, 0.5], [0, 1]
    ml._quicksort(d, p, 0, 1, False)
    assert p == [1, 0]
    d, p = [0.3, 0.2, 0.1], [0, 1, 2]
    ml._quicksort(d, p, 0, 2, False)
    assert p == [0, 1, 2]


def test_gaussian_kernel_and_smoothing_order():
    k = ml.gaussian_kernel(9, 3.0)
    assert k.dtype == np.float32 and abs(float(k.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(k, k[::-1])
    img = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(ml.smooth(img, 0, 3.0), img)
    flat = np.full((9, 4), np.float32(0.3))
    assert np.abs(ml.smooth(flat, 4, 3.0) - 0.3).max() < 1e-6  # narrower than the kernel: the replicate border


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------

def test_ids_and_struct_layout_match_c(tmp_path):
    inc = os.path.join(ROOT, "include")
    src = tmp_path / "ml_abi.c"
    ids = ("35", "36", "BGS_MULTILAYER", "BGS_ALGO_LAST", "(int)BGS_ALGO_LAST + 1")
    known = ", ".join("BGS_ALGO_KNOWN(%s)" % i for i in ids)
    offs = ", ".join("offsetof(bgs_multilayer_params, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%d %d %zu %d %d %d %d %zu' + " %d" * len(ids) + " %zu" * len(FIELDS)
                   + '\\n", (int)BGS_ALGO_LAST, (int)BGS_MULTILAYER, sizeof(bgs_multilayer_params), (int)BGS_MULTILAYER_MAX_HALF_SIZE, (int)BGS_ALGO_COUNT, (int)BGS_ALGO_END, (int)BGS_ALGO_LIMIT, sizeof(bgs_params), '
                   + known + ", " + offs + ");return 0;}\n")
    exe = tmp_path / "ml_abi"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert v[0] == capi.ALGO_LAST > capi.MULTILAYER  # header and binding agree on the moving marker; its value is not pinned
    assert v[1] == 36 == capi.MULTILAYER
    assert v[2] == C.sizeof(PARAMS) == 96 and v[3] == capi.MULTILAYER_MAX_HALF_SIZE == 8
    assert v[4:7] == [21, 26, 28]  # the frozen markers
    assert v[7] == C.sizeof(capi.BgsParams) == 336  # bgs_params did not grow
    assert v[8:8 + len(ids)] == [1, 1, 1, 0, 0]  # one past the last id is unknown, symbolically
    assert v[8 + len(ids):] == [getattr(PARAMS, f).offset for f in FIELDS] == list(range(0, 96, 4))
    assert FIELDS[1:] == ml.FIELDS
    text = open(os.path.join(ROOT, "tracking_amd", "capi.py")).read()
    assert len(set(re.findall(r"^ALGO_LAST = (\d+)", text, re.M))) == 1


def test_unknown_ids_stay_unknown_and_the_new_one_is_known():
    p = capi.BgsParams()
    p.struct_size = C.sizeof(capi.BgsParams)
    for bad in (capi.ALGO_LAST, capi.ALGO_LAST + 1):
        assert capi.lib().bgs_default_params(bad, C.byref(p)) == capi.ERR_INVALID, bad
        h = C.c_void_p()
        assert capi.lib().bgs_create(bad, None, 0, 1, C.byref(h)) == capi.ERR_INVALID and b"unknown algorithm" in capi.lib().bgs_last_error()
    assert capi.lib().bgs_default_params(capi.MULTILAYER, C.byref(p)) == capi.OK


def test_default_multilayer_params():
    p = capi.multilayer_default_params()
    assert p.struct_size == 96
    for k, v in ml.DEFAULTS.items():
        want = v if k in ml.INT_FIELDS else float(np.float32(v))
        assert getattr(p, k) == want, k
    assert capi.lib().bgs_multilayer_default_params(None) == capi.ERR_INVALID


def refused(rows=0, cols=0, ch=3, **kw):
    p = capi.multilayer_default_params(**kw)
    rc = capi.lib().bgs_multilayer_check(C.byref(p), rows, cols, ch)
    return rc, capi.lib().bgs_last_error().decode()


@pytest.mark.parametrize("kw", [dict(max_mode_num=0), dict(max_mode_num=6), dict(pattern_neig_half_size=9), dict(pattern_neig_gaus_sigma=0.0),
                                dict(pattern_neig_half_size=0, pattern_neig_gaus_sigma=-1.0), dict(texture_weight=float("nan")), dict(frame_duration=float("inf")),
                                dict(bg_prob_threshold=float("nan")), dict(min_noised_angle=float("-inf")), dict(learn_init_mode_weight=float("nan"))])
def test_check_refuses_bad_parameters_without_a_device(kw):
    rc, msg = refused(**kw)
    assert rc == capi.ERR_UNSUPPORTED and ml.CLASS_NAME in msg, (kw, msg)


def test_check_accepts_what_the_reference_accepts_and_refuses_gray_frames():
    assert capi.lib().bgs_multilayer_check(None, 0, 0, 0) == capi.OK
    for kw in (dict(pattern_neig_half_size=-1, pattern_neig_gaus_sigma=0.0), dict(texture_weight=0.0), dict(texture_weight=-1.0), dict(max_mode_num=1),
               dict(pattern_neig_half_size=8), dict(weight_updating_constant=0.0)):
        assert refused(**kw)[0] == capi.OK, kw
    assert refused(12, 16, 3)[0] == capi.OK
    rc, msg = refused(12, 16, 1)
    assert rc == capi.ERR_UNSUPPORTED and ml.CLASS_NAME in msg and "3-channel" in msg
    bad = capi.multilayer_default_params()
    bad.struct_size = 92
    assert capi.lib().bgs_multilayer_check(C.byref(bad), 0, 0, 3) == capi.ERR_INVALID


def test_host_computed_constants_equal_the_fixture_s_bits():
    bits = (C.c_uint32 * 2)()
    assert capi.lib().bgs_multilayer_constants(None, bits) == capi.OK
    for case, r in ml.load().items():
        p = capi.multilayer_default_params(**r["params"])
        assert capi.lib().bgs_multilayer_constants(C.byref(p), bits) == capi.OK
        assert [int(bits[0]), int(bits[1])] == [int(r["consts"][0]), int(r["consts"][1])], case
    m = ml.Model({}, 4, 4)
    assert m.constants_bits()[1] == int(ml.load()["defaults"]["consts"][1])  # (float)(10.0 / 180.0 * PI) with the float PI macro


# ---- host layer --------------------------------------------------------------------------------------------------------------------------

def test_host_layer_compiles():
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(HOST, "FrameProcessor.cpp")], check=True)
