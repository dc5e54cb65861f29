"""DPZivkovicAGMMBGS, DPGrimsonGMMBGS, DPWrenGABGS, DPMeanBGS, DPAdaptiveMedianBGS (USTC_BGS types 9-13) on the CPU: the restatement
the HIP kernels are compared with (oracle/dp_oracle.c) against the outputs of the reference's own model files
(tests/golden/dp_ref_*.npz, written by tests/golden/make_dp_ref.py: pinned) - masks and every stored plane bit for bit -, against
the live reference build where oracle/_ref holds it, what the fixtures claim to cover, and the refused parameters."""
import ctypes as C

import numpy as np
import pytest

import dp_ref
from oracle import pyoracle
from tracking_amd import capi

ALL = [(cls, case) for cls in dp_ref.CLASSES for case in dp_ref.cases(cls)]
IDS = ["%s-%s" % cc for cc in ALL]


@pytest.mark.parametrize("cls,case", ALL, ids=IDS)
def test_oracle_matches_reference_fixture(cls, case):
    r = dp_ref.load(cls)[case]
    masks, planes = dp_ref.oracle_run(cls, r["params"], r["frames"], r["planes"])
    bad = np.nonzero((masks != r["masks"]).reshape(len(masks), -1).any(1))[0]
    assert not len(bad), "frames %s differ, %d pixels in all" % (bad[:5], int((masks != r["masks"]).sum()))
    for name, want in r["planes"].items():
        assert dp_ref.same_bits(planes[name], want), "%s: %d entries differ in their bits" % (name, int((planes[name].view(np.uint8) != want.view(np.uint8)).sum()))


def test_fixture_files_hold_exactly_the_declared_cases():
    for cls in dp_ref.CLASSES:
        got = dp_ref.load(cls)
        want = dp_ref.cases(cls)
        assert list(got) == list(want), cls
        for case, p in want.items():
            assert got[case]["params"] == p, (cls, case)
            n = got[case]["frames"].shape[1] * got[case]["frames"].shape[2]
            assert bool(got[case]["planes"]) == (n <= dp_ref.PLANE_PIXELS * 1.05), (cls, case)
            assert n < 8000 and len(got[case]["frames"]) < 80


@pytest.mark.parametrize("cls,case", ALL, ids=IDS)
def test_oracle_matches_live_reference_build(cls, case):
    """Where oracle/_ref/ref_dp_cli exists the reference itself is asked on the same input, with a poison byte of its own: it
    must give the fixture (the fixture is current) and so the oracle."""
    if not pyoracle.ref_dp_available():
        return
    r = dp_ref.load(cls)[case]
    masks, model = pyoracle.ref_dp_clip(cls, r["frames"], planes=True, poison=0x5A, **dp_ref.ref_kwargs(cls, r["params"]))
    assert np.array_equal(masks, r["masks"])
    for name, want in r["planes"].items():
        assert dp_ref.same_bits(model[name], want), name
    omasks, oplanes = dp_ref.oracle_run(cls, r["params"], r["frames"], model)
    assert np.array_equal(omasks, masks)
    for name in model:  # every plane, also of the cases too large to store
        assert dp_ref.same_bits(oplanes[name], model[name]), name


def test_default_and_shape_cases_are_not_trivial():
    for cls in dp_ref.CLASSES:
        cases = dp_ref.load(cls)
        m = cases["default"]["masks"]
        share = (m != 0).mean(axis=(1, 2))
        assert len(m) == 72 and m.shape[1:] == (80, 96)
        # not trivial: both values occur, most frames hold some foreground, and the scene changes show as different shares
        assert 0.01 < share.mean() < 0.99 and (share > 0).mean() > 0.8 and share.max() - share.min() > 0.05, (cls, share.mean())
        assert cases["default"]["params"] == dict(dp_ref.DEFAULTS[cls], input="long72")
        for case, shape in (("ragged", (10, 37, 53)), ("tile", (12, 16, 64)), ("tiny5x7", (12, 5, 7)), ("tiny1x1", (12, 1, 1))):
            assert cases[case]["masks"].shape == shape
        assert (37 * 53) % 4 and (37 * 53) % 256 and 16 * 64 == 4 * 256
        for a, b in (("ragged", "ragged_o1"), ("ragged_o1", "ragged_o2")):  # windows of one clip, one frame apart
            assert np.array_equal(cases[a]["frames"][1:], cases[b]["frames"][:-1])
            assert not np.array_equal(cases[a]["masks"][1:], cases[b]["masks"][:-1])
        assert set(np.unique(cases["ties"]["frames"])) <= {0, 128, 255}
        assert cases["ties"]["masks"].any() and not cases["ties"]["masks"].all()


@pytest.mark.parametrize("cls", ["ziv", "grim"])
def test_gmm_cases_fill_k_modes_and_replace_one(cls):
    cases = dp_ref.load(cls)
    F = dp_ref.FIELDS[cls]
    for case, K in (("modes_k1", 1), ("modes_k2", 2), ("modes", 3), ("modes_k4", 4), ("modes_k5", 5), ("modes_ties", 3)):
        r = cases[case]
        assert r["params"]["gaussians"] == K
        nm = r["planes"]["nmodes"]
        assert nm.max() == K and (nm == K).mean() > 0.2, (case, np.bincount(nm))
        # a pixel of the clip dwells on four colours of its own: with K < 4 the fourth finds every slot taken and replaces the last
        f = r["frames"].reshape(len(r["frames"]), -1, 3).astype(np.int32)
        jumps = (np.abs(np.diff(f, axis=0)).max(-1) > 40).sum(0)
        assert (jumps[nm == K] >= K).any()
        modes = r["planes"]["modes"].reshape(K, F, -1)
        assert np.isfinite(modes).all()
        w = modes[:, 4]
        full = nm == K
        assert np.allclose(w[:, full].sum(0), 1, atol=1e-5)  # weights of the used modes are normalised
        key = modes[:, 5] if cls == "grim" else w
        assert (np.diff(key[:, full], axis=0) <= 0).all()  # and sorted, largest first


def test_grimson_fixtures_hold_sort_ties_and_say_which_sqrt_built_them():
    """qsort's order of modes with equal `significants` is a property of the C library, the sqrt overload one of the headers: the
    fixture build's answers are recorded, and the cases that could tell a different answer apart are counted."""
    env = dp_ref.environment("grim")
    assert env["sqrt_overload"] == "sqrt(float) -> float"
    assert env["sqrt_double_changes_cases"], "no fixture case tells the float overload of sqrt from the double one"
    cases = dp_ref.load("grim")
    # `modes` (default alpha 0.01) meets none: keys are equal only where rounding has made weights equal, which takes an alpha below
    # float's epsilon - `ties` and `modes_ties` run with 1e-8, where every mode after the first keeps weight alpha and variance 36
    for case in ("ties", "modes_ties"):
        pyoracle.dp_grimson_sort_ties(reset=True)
        dp_ref.oracle_run("grim", cases[case]["params"], cases[case]["frames"])
        ties = pyoracle.dp_grimson_sort_ties(reset=True)
        print("%s: %d sorts met equal keys" % (case, ties))
        assert ties > 0, case


def test_median_threshold_wraps_show_in_the_fixtures():
    """AdaptiveMedianParams holds unsigned char thresholds: low = threshold mod 256, high = 2 * low mod 256."""
    c = dp_ref.load("median")
    m = lambda t: c["t%d" % t]["masks"]  # noqa: E731
    share = lambda t: float((m(t) != 0).mean())  # noqa: E731
    assert not np.array_equal(m(130), m(100))  # high 4 against high 200
    assert share(130) > 0.5 > share(100)
    assert np.array_equal(m(256), m(0)) and np.array_equal(m(300), m(44))
    assert not np.array_equal(m(128), m(127)) and share(128) > share(127)  # high 0 against high 254
    assert np.array_equal(m(-1), m(255)) and np.array_equal(m(255), m(127))  # low 255 -> high 510 mod 256 = 254, as 127 gives
    assert not np.array_equal(m(200), m(100))  # high 144
    for t in (130, 300):
        assert c["tile_t%d" % t]["masks"][1:].mean() > 100 and c["ragged_t%d" % t]["masks"][1:].mean() > 100
    for a, b in (("rate1", "rate2"), ("rate2", "rate7")):
        assert not np.array_equal(c[a]["planes"]["median"], c[b]["planes"]["median"])


def test_mean_threshold_wraps_show_in_the_fixtures():
    c = dp_ref.load("mean")
    assert not c["t-1"]["masks"].any()  # unsigned int: -1 -> 4 294 967 295, nothing is foreground
    assert c["t0"]["masks"][1:].mean() > 250 and 0 < c["t5000"]["masks"].mean() < c["t0"]["masks"].mean()
    assert not np.array_equal(c["alpha05"]["planes"]["mean"], c["alpha09"]["planes"]["mean"])


@pytest.mark.parametrize("cls", ["wren", "mean", "median"])
def test_learning_frames_zero_equals_its_twin(cls):
    c = dp_ref.load(cls)
    assert c["learn0"]["params"]["learning_frames"] == 0 and c["ragged"]["params"]["learning_frames"] == 30
    assert np.array_equal(c["learn0"]["frames"], c["ragged"]["frames"])
    assert np.array_equal(c["learn0"]["masks"], c["ragged"]["masks"]) and c["ragged"]["masks"].any()


@pytest.mark.parametrize("algo,name", [(capi.DP_MEAN, b"DPMeanBGS"), (capi.DP_ADAPTIVE_MEDIAN, b"DPAdaptiveMedianBGS")])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf"), 2147483648.0, -2147483904.0, 3e38])
def test_refused_parameters(algo, name, value):
    """The two wrappers hold `int threshold`; bgs_params carries it as a float, so a value no int holds is refused."""
    p = capi.default_params(algo)
    p.dp_threshold = value
    h = C.c_void_p()
    assert capi.lib().bgs_create(algo, C.byref(p), 0, 1, C.byref(h)) == capi.ERR_UNSUPPORTED
    assert name in capi.lib().bgs_last_error()
    with pytest.raises(RuntimeError):  # the oracle refuses it as well (at its first frame)
        o = pyoracle.Oracle(algo, params=p)
        o.process(np.zeros((2, 2, 3), np.uint8), want_bg=False)


def test_accepted_thresholds_at_the_ends_of_int():
    for algo in (capi.DP_MEAN, capi.DP_ADAPTIVE_MEDIAN):
        for value in (-2147483648.0, 2147483520.0, -1.0, 300.0):
            p = capi.default_params(algo)
            p.dp_threshold = value
            o = pyoracle.Oracle(algo, params=p)
            assert o.process(np.zeros((2, 2, 3), np.uint8), want_bg=False)[0] is not None
