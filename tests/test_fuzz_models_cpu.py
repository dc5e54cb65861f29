"""The fuzz of the 16 reference-pinned model classes (tools/fuzz_parity.py `models`, tests/model_refs.py), checked without a GPU: the
old table still draws the cases it always drew, a draw is pure and deterministic, the fixed slices of tests/test_gpu_20_fuzz_models.py
cover what each class needs, the checkers report planted defects, and the slices' inputs tell a restatement from the same restatement
one parameter step away."""
import functools
import json
import os
import sys
import time

import numpy as np
import pytest

import model_refs as mr
from tools import fuzz_parity as fp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLICES = {s[0]: s for s in mr.SLICES}


# ---- the old table -------------------------------------------------------------------------------------------------------------------

def test_old_table_draws_the_cases_it_always_drew():
    """20 seeds of tests/test_gpu_08_fuzz.py against the draws recorded from the tool as it was before draw_case / run_case were split
    (its one_case run with the engine constructor stubbed out): class, geometry, streams, frames, parameter dict."""
    rec = json.load(open(os.path.join(GOLDEN, "fuzz_draws.json")))
    assert len(rec) == 20 and any(r["big"] for r in rec)
    for r in rec:
        c = fp.draw_case(np.random.default_rng(r["seed"]), r["seed"], "all", big=r["big"])
        params = {k: v for k, v in c["params"].items() if k != "sparse"}  # the MOG2 kernel choice was drawn after the engine existed
        assert (c["name"], fp.ALL[c["name"]], c["H"], c["W"], c["S"], c["T"], params) == (r["name"], r["algo"], r["H"], r["W"], r["S"], r["T"], r["params"]), r["seed"]
        assert len(c["inputs"]) == c["S"] and sum(st["n"] for st in c["steps"]) == c["T"]


def test_a_draw_is_pure_and_deterministic(monkeypatch):
    """No torch, no engine; the same seed gives the same description (JSON text, so every nested value counts)."""
    def boom(*a, **k):
        raise AssertionError("draw_case must not construct an engine")
    monkeypatch.setattr(fp, "Engine", boom)
    monkeypatch.setattr("tracking_amd.Engine", boom)
    monkeypatch.setattr("tracking_amd.capi.lib", boom)
    monkeypatch.setitem(sys.modules, "torch", None)  # `import torch` now raises
    for table, big, seeds in (("all", False, range(41000, 41030)), ("all", True, range(63000, 63010)), ("models", False, range(700000, 700040)),
                              ("models", True, range(800000, 800008)), ("lb", False, range(5, 15)), (["T2FGMM_UV"], False, range(3))):
        for seed in seeds:
            a = fp.draw_case(np.random.default_rng(seed), seed, table, big=big)
            b = fp.draw_case(np.random.default_rng(seed), seed, table, big=big)
            assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True), (table, seed)
            assert a["seed"] == seed and sum(st["n"] for st in a["steps"]) == a["T"]
            if table == "lb":
                assert a["family"] == "lb"


# ---- the slices ----------------------------------------------------------------------------------------------------------------------

def test_the_slices_of_the_first_14_classes_keep_their_seeds():
    """IndependentMultimodalBGS and MultiLayerBGS sort into the middle of the class list; they take indices 14 and 15, and the 41
    slices that were there before them are the tuples they were (tests/golden/fuzz_model_slices.json, recorded from the table of 14)."""
    rec = [tuple([r[0], tuple(r[1])] + r[2:]) for r in json.load(open(os.path.join(GOLDEN, "fuzz_model_slices.json")))]
    assert len(rec) == 41 and len({r[1] for r in rec}) == 14
    late = {(mr.im.CLASS_NAME,), (mr.ml.CLASS_NAME,)}
    assert [s for s in mr.SLICES if s[1] not in late] == rec
    mine = [s for s in mr.SLICES if s[1] == (mr.im.CLASS_NAME,)]
    assert [(s[2], s[3], s[4]) for s in mine] == [(False, 714000, 36), (True, 814000, 2), (True, 814002, 2), (True, 814004, 2), (True, 814006, 2)]
    mine = [s for s in mr.SLICES if s[1] == (mr.ml.CLASS_NAME,)]
    assert [(s[2], s[3], s[4]) for s in mine] == [(False, 715000, 36), (True, 815000, 4), (True, 815004, 4)]
    assert len({s[0] for s in mr.SLICES}) == len(mr.SLICES) == 49


@functools.lru_cache(maxsize=None)
def drawn(slice_id):
    _, classes, big, first, count = SLICES[slice_id]
    return mr.slice_cases(first, count, classes, big)


def accepted(cases):
    return [c for c in cases if mr.BY_CLASS[c["name"]].refusal(c["name"], c["params"]) is None]


def lively(case, outs):
    """A compared frame whose restatement mask has at least 5 % foreground and at least 5 % background."""
    for per_stream in outs:
        for fg, _, ignore in per_stream:
            if fg is not None and 0.05 <= float((fg != 0).mean()) <= 0.95:
                return True
    return False


@functools.lru_cache(maxsize=None)
def restated(slice_id):
    """(seconds, [(case, lively, stats)]) of the slice's accepted cases: the restatement side of the GPU test, run once."""
    t0 = time.time()
    out = []
    for c in accepted(drawn(slice_id)):
        outs, _, stats = mr.reference_run(c)
        out.append((c, lively(c, outs), stats))
    return time.time() - t0, out


@pytest.mark.parametrize("name", mr.MODELS)
def test_slices_cover_what_the_class_needs(name):
    ad = mr.BY_CLASS[name]
    small = [c for sid in mr.slices_of(name, False) for c in drawn(sid)]
    big = [c for sid in mr.slices_of(name, True) for c in drawn(sid)]
    assert all(c["name"] == name for c in small + big)
    for c in small + big:  # the draw's own record of a refused value agrees with the adapter's table
        assert (c["bad"] is not None) == (ad.refusal(name, c["params"]) is not None), c["seed"]
    a_small, a_big = accepted(small), accepted(big)
    assert len(a_small) >= 24 and len(a_big) >= 6, (len(a_small), len(a_big))
    ok = a_small + a_big
    modes = [c["mode"] for c in ok]
    assert all(modes.count(m) >= 2 for m in mr.MODES), {m: modes.count(m) for m in mr.MODES}
    assert any(c["H"] == min(ad.h_small) for c in ok), "the smallest accepted height"
    assert any(c["H"] * c["W"] % 64 for c in ok) and any(c["H"] * c["W"] % 64 == 0 for c in ok)
    assert any(c["S"] == 3 for c in ok)
    assert any(st["resets"] for c in ok for st in c["steps"]), "a reset"
    assert any(c["switch"] for c in ok), "a parameter switch"
    if type(ad).draw_bad is not mr.Adapter.draw_bad:  # Texture has no parameter and VuMeter's setters replace a bad value: nothing to refuse
        assert len(small + big) > len(ok), "a refused parameter"
    else:
        assert name in ("DPTexture", "VuMeter")
    if ad.family in ("lb", "t2f"):
        assert any(st["m"] == "clip" and st["n"] >= 9 for c in ok for st in c["steps"]), "a clip call of 9 or more frames"
    if ad.family == "texture":  # below the 15 x 15 neighbourhood and above it
        assert any(min(c["H"], c["W"]) < 15 for c in ok) and any(min(c["H"], c["W"]) >= 15 for c in ok)
    if ad.family == "vumeter":
        assert any(min(c["H"], c["W"]) < 5 for c in ok)
    secs = {}
    for is_big in (False, True):
        rows = []
        for sid in mr.slices_of(name, is_big):
            secs[sid], r = restated(sid)
            rows += r
        sized = [live for c, live, _ in rows if c["H"] * c["W"] >= 20]
        assert 2 * sum(sized) >= len(sized), "%s: %d of %d %s cases have a frame with 5 %% foreground and 5 %% background" % (name, sum(sized), len(sized), "big" if is_big else "small")
        if ad.family == "eigen":
            assert 5 * sum(c["redraws"] > 0 for c, _, _ in rows) <= len(rows), "more than a fifth of the draws had to be redrawn"
            for c, _, st in rows:
                assert st["gaps"] and all(g >= mr.en.EIGENGAP for g in st["gaps"]) and st["band"] <= mr.en.BAND_SHARE * st["detected"], c["seed"]
        if ad.family == "imbs":  # the area filter removes something of a compared frame's 255-plane in at least half of the sized cases
            cut = [st.get("filtered", 0) > 0 for c, _, st in rows if c["H"] * c["W"] >= 20]
            assert 2 * sum(cut) >= len(cut), "%d of %d %s cases have a frame of which the area filter removes pixels" % (sum(cut), len(cut), "big" if is_big else "small")
            assert all(c["redraws"] == 0 for c, _, _ in rows)  # no draw is redrawn: parity is claimed on every input
    if ad.family == "imbs":  # labels 180 and 80 occur, frames below 3 x 3 (no interior: the filter leaves nothing) and a morphology case too
        every = [(c, st) for sid in mr.slices_of(name, False) + mr.slices_of(name, True) for c, _, st in restated(sid)[1]]
        assert sum(st.get(180, 0) > 0 for _, st in every) >= 3 and sum(st.get(80, 0) > 0 for _, st in every) >= 3
        assert any(min(c["H"], c["W"]) < 3 for c, _ in every) and any(c["W"] == 3 for c, _ in every) and any(c["params"]["morphologicalFiltering"] for c, _ in every)
        assert {r["kind"] for c, _ in every for r in c["inputs"]} == set(ad.kinds)
        assert any(c["H"] * c["W"] > 4 * 256 and c["H"] * c["W"] % 256 for c, _ in every) and max(c["H"] * c["W"] for c, _ in every) <= 65 * 131
    if ad.family == "multilayer":
        every = [(c, st) for sid in mr.slices_of(name, False) + mr.slices_of(name, True) for c, _, st in restated(sid)[1]]
        half = lambda c: c["params"]["pattern_neig_half_size"]
        assert {half(c) for c, _ in every} == set(range(-1, 9)), "every half size"
        assert any(half(c) == 8 and min(c["H"], c["W"]) < 8 for c, _ in every), "the largest halo on a frame smaller than it"
        assert any(half(c) == 8 and c["W"] in (31, 32, 33) for c, _ in every), "the largest halo at the smoothing tile's edge"
        assert {c["params"]["max_mode_num"] for c, _ in every} == {1, 2, 3, 4, 5}
        assert any(c["params"]["texture_weight"] <= 0 for c, _ in every)
        assert any(c["H"] == 1 and c["W"] > 1 for c, _ in every) and any(c["W"] == 1 and c["H"] > 1 for c, _ in every) and any(c["H"] == c["W"] == 1 for c, _ in every)
        after = lambda c: c["params"]["detect_after"]
        # a reset past detect_after sends one stream back to learning beside detecting ones: a call holds different launch keys
        assert sum(c["S"] >= 2 and after(c) > 0 and any(st["resets"] and st["t"] > after(c) for st in c["steps"]) for c, _ in every) >= 3
        assert sum(any(st["m"] == "clip" and st["n"] >= 2 and st["t"] < after(c) < st["t"] + st["n"] for st in c["steps"]) for c, _ in every) >= 2, "the switch inside a clip call"
        total = {k: sum(st.get(k, 0) for _, st in every) for k in mr.ml.COUNTERS}
        assert all(v > 0 for v in total.values()), total
        for k in ("removal_second", "stale_decay_matched"):
            assert sum(st.get(k, 0) > 0 for _, st in every) >= 3, k
        assert {r["kind"] for c, _ in every for r in c["inputs"]} == set(ad.kinds)
        assert all(c["redraws"] == 0 for c, _ in every)  # no draw is redrawn: parity is claimed on every input
    print("%s: restatement side of each slice, seconds: %s" % (name, {k: round(v, 1) for k, v in secs.items()}))


@pytest.mark.parametrize("name", mr.MODELS)
def test_inputs_tell_a_restatement_from_its_neighbour(name):
    """restatement(p) against restatement(p') over the first 6 accepted cases of the class's small slice, p' one smallest step away in
    one parameter, through the GPU test's own comparison functions: at least one case must mismatch, or the slice is too tame to
    notice a subtly wrong kernel."""
    ad = mr.BY_CLASS[name]
    key, step, default = ad.step_of[name]
    caught = 0
    for c in accepted(drawn(mr.slices_of(name, False)[0]))[:6]:
        frames = mr.build_inputs(c)
        a, refs_a, _ = mr.reference_run(c, frames)
        p2 = dict(c["params"])
        p2[key] = step(p2.get(key, default))
        assert ad.refusal(name, p2) is None, p2
        b, refs_b, _ = mr.reference_run(c, frames, params=p2)
        try:
            for s in range(c["S"]):
                for t in range(c["T"]):
                    (fa, ba, ig), (fb, bb, _) = a[s][t], b[s][t]
                    assert (fa is None) == (fb is None)
                    if fa is not None:
                        mr.check_mask(fb, fa, "mask", ig)
                    if ba is not None:
                        mr.check_background(bb, ba, "background")
                want = ad.normalise(name, refs_a[s].planes())
                mr.check_planes(ad.normalise(name, refs_b[s].planes()), want, ad.tols.get(name, {}), "planes")
        except AssertionError:
            caught += 1
    assert caught >= 1, "%s: %s one step further changes nothing the comparison sees" % (name, key)


# ---- the checkers --------------------------------------------------------------------------------------------------------------------

def _model():
    rng = np.random.default_rng(3)
    return {"mu": rng.uniform(0, 255, (40, 3)), "w": rng.uniform(0, 1, (40, 3)).astype(np.float32), "k": rng.integers(0, 4, 40).astype(np.int32)}


def test_checkers_report_planted_defects():
    rng = np.random.default_rng(1)
    mask = np.where(rng.random((9, 13)) < 0.3, 255, 0).astype(np.uint8)
    bad = mask.copy()
    bad[4, 5] ^= 255
    mr.check_mask(mask.copy(), mask, "same")
    with pytest.raises(AssertionError, match="1 mask pixels"):
        mr.check_mask(bad, mask, "one flipped mask pixel")
    ignore = np.zeros(mask.shape, bool)
    ignore[4, 5] = True
    mr.check_mask(bad, mask, "inside the band", ignore)
    ignore[4, 5], ignore[4, 6] = False, True
    with pytest.raises(AssertionError):
        mr.check_mask(bad, mask, "beside the band", ignore)
    bg = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    worse = bg.copy()
    worse[0, 0, 2] ^= 1
    mr.check_background(bg.copy(), bg, "same")
    with pytest.raises(AssertionError, match="1 background bytes"):
        mr.check_background(worse, bg, "one flipped background byte")
    want = _model()
    tols = {"mu": 2e-12}
    mr.check_planes({k: v.copy() for k, v in want.items()}, want, tols, "same")
    for plane, change in (("w", lambda a: np.nextafter(a, np.float32(2))), ("k", lambda a: a + 1)):  # one ulp / one count in an exact plane
        got = {k: v.copy() for k, v in want.items()}
        got[plane][7] = change(got[plane][7])
        with pytest.raises(AssertionError, match="plane %s" % plane):
            mr.check_planes(got, want, tols, "exact plane")
    got = {k: v.copy() for k, v in want.items()}
    got["mu"][3, 1] += 0.5 * tols["mu"]  # inside the tolerance (mu < 256: an ulp is 2.8e-14)
    mr.check_planes(got, want, tols, "half a tolerance")
    got["mu"][3, 1] = want["mu"][3, 1] + 2 * tols["mu"]
    with pytest.raises(AssertionError, match="plane mu"):
        mr.check_planes(got, want, tols, "twice the tolerance")
    for plane in ("mu", "w"):  # NaN against a number, in a tolerance plane and in an exact one, either way round
        for a, b in ((np.nan, None), (None, np.nan), (np.inf, None), (np.inf, -np.inf)):
            got, ref = {k: v.copy() for k, v in want.items()}, {k: v.copy() for k, v in want.items()}
            if a is not None:
                got[plane][2] = a
            if b is not None:
                ref[plane][2] = b
            with pytest.raises(AssertionError, match="plane %s" % plane):
                mr.check_planes(got, ref, tols, "NaN / infinity against a number")
    assert mr.count_exact(np.float32([0.0]), np.float32([-0.0])) == 1  # raw bits: the zeros differ


def test_checkers_do_not_report_equal_nans_and_equal_infinities():
    want = _model()
    for plane in ("mu", "w"):
        got, ref = {k: v.copy() for k, v in want.items()}, {k: v.copy() for k, v in want.items()}
        for d in (got, ref):
            d[plane][2, 0], d[plane][5, 1], d[plane][6, 2] = np.nan, np.inf, -np.inf
        mr.check_planes(got, ref, {"mu": 2e-12}, "equal NaNs and infinities")
    a = np.array([np.nan], np.float32)
    b = (a.view(np.uint32) | 1).view(np.float32)  # another payload: still a NaN
    assert np.isnan(b[0]) and a.view(np.uint32)[0] != b.view(np.uint32)[0] and mr.count_exact(a, b) == 0


def test_packed_words_have_zero_tail_bits():
    m = np.full((5, 7), 255, np.uint8)
    w = mr.words_of(m)
    assert w.shape == (1,) and int(w[0]) == (1 << 35) - 1
    assert mr.words_of(np.zeros((8, 16), np.uint8)).shape == (2,)
