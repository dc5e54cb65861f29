"""One adapter per model family for tools/fuzz_parity.py's `models` table (not a test module): the 16 classes that are pinned to
reference-built fixtures and restated in numpy (kde_numpy, dp2_numpy, lb_numpy, vumeter_numpy, fuzzy_numpy, t2f_numpy, eigen_numpy,
imbs_numpy, multilayer_numpy).

An adapter draws parameters (and, rarely, one the engine must refuse: `refusal()` is the table), names the
input generators of its family, builds the restatement of one stream (`make_ref`: a fresh one per stream and after every
reset_stream), says which parameters a running stream follows (`follow`) and under which contract the model is compared at the end
(`tols`: a plane that is not named there is compared bit for bit).  Everything up to `reference_run` needs neither torch nor an
engine; `make_engine` / `apply` are the only functions that touch the library.

The checkers at the top take arrays, so tests/test_fuzz_models_cpu.py can plant defects in them.  NaN against NaN and equal
infinities count as equal, in exact and in tolerance comparisons alike."""
import numpy as np

import dp2_numpy as dn
import eigen_numpy as en
import fuzzy_numpy as fz
import imbs_masks as mk
import imbs_numpy as im
import kde_numpy as kn
import lb_numpy as ln
import multilayer_numpy as ml
import multilayer_scenes as msc
import t2f_numpy as tn
import vumeter_numpy as vn
from tracking_amd import capi

MODES = ("host", "submit", "batch", "ranges", "clip", "mixed")
FG_MARK, BG_MARK = 7, 9  # what the output buffers hold before a call: an untouched output still shows it
H_SMALL, W_SMALL = [1, 7, 16, 33, 64], [3, 64, 70, 128, 200]          # the lists of the old table
H_BIG, W_BIG = [33, 65, 97, 130, 200], [64, 97, 131, 257, 320]


# ---- checkers (arrays in, AssertionError out) -------------------------------------------------------------------------------------

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def count_exact(got, want):
    """Elements whose bits differ.  NaN on both sides is equal whatever its payload; equal infinities have equal bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "shape / type %s %s against %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    bad = _bits(got) != _bits(want)
    if got.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    return int(bad.sum())


def count_within(got, want, tol):
    """Elements further than tol apart.  Equal values (infinities included) and NaN on both sides are equal; NaN or an infinity
    against anything else is a difference."""
    a, b = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert a.shape == b.shape, "shape %s against %s" % (a.shape, b.shape)
    with np.errstate(invalid="ignore"):
        ok = (a == b) | (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)
    return int((~ok).sum())


def check_mask(got, want, where, ignore=None):
    bad = np.asarray(got) != np.asarray(want)
    if ignore is not None:
        bad &= ~ignore
    assert not bad.any(), "%s: %d mask pixels differ" % (where, int(bad.sum()))


def check_background(got, want, where):
    got = np.asarray(got).reshape(np.asarray(want).shape)
    assert np.array_equal(got, want), "%s: %d background bytes differ" % (where, int((got != want).sum()))


def check_planes(got, want, tols, where):
    """Every plane of `want` against the same plane of `got`: within tols[name] where the contract has a tolerance, else bit for bit."""
    for name, w in want.items():
        tol = tols.get(name)
        n = count_exact(got[name], w) if tol is None else count_within(got[name], w, tol)
        assert n == 0, "%s: plane %s, %d of %d values differ (%s)" % (where, name, n, np.asarray(w).size, "exact" if tol is None else "tolerance %g" % tol)


def words_of(mask):
    """(H*W + 63) // 64 packed words of a byte mask, tail bits zero."""
    packed = np.packbits(np.asarray(mask).reshape(-1) != 0, bitorder="little")
    w = np.zeros((mask.size + 63) // 64 * 8, np.uint8)
    w[:len(packed)] = packed
    return w.view(np.uint64)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def _clip(kind, T, H, W, seed, quiet):
    if kind.startswith("synth_"):
        from tools import synth
        k = kind[6:]
        return synth.random_frames(T, H, W, 3, seed=seed) if k == "random" else synth.numpy_frames(k, T, H, W, seed=seed)
    return {"lb_noisy": lambda: ln.noisy_clip(T, H, W, seed, box=0.15), "lb_modes": lambda: ln.modes_clip(T, H, W, seed), "lb_tie": lambda: ln.tie_clip(T, H, W, seed),
            "dp2_scene": lambda: dn.scene_clip(T, H, W, seed, box=0.15), "dp2_tie": lambda: dn.tie_clip(T, H, W, seed), "dp2_texture": lambda: dn.texture_clip(T, H, W, seed),
            "t2f_scene": lambda: tn.scene_clip(T, H, W, seed), "t2f_corners": lambda: tn.corners_clip(T, H, W, seed),
            "vu_box": lambda: vn.bgr(T, H, W, seed), "vu_leave": lambda: np.repeat(vn.leave(T, H, W, seed)[..., None], 3, axis=-1),
            "eigen_pca": lambda: en.pca_clip(T, H, W, seed, quiet), "imbs_box": lambda: im.clip("box", T, H, W, seed), "imbs_persist": lambda: im.clip("persist", T, H, W, seed),
            "imbs_shadow": lambda: _imbs_event("shadow", 2, T, H, W, seed, quiet), "imbs_holes": lambda: _imbs_event("holes", 2, T, H, W, seed, quiet),
            "imbs_sudden": lambda: _imbs_event("sudden", 3, T, H, W, seed, quiet), "imbs_inject": lambda: mk.fuzz_clip(T, H, W, seed, quiet),
            "ml_scripted": lambda: msc.frames_of("scripted", H, W, T, seed), "ml_dark": lambda: msc.frames_of("dark", H, W, T, seed),
            "ml_block": lambda: msc.frames_of("static_block", H, W, T, seed), "ml_scaled": lambda: msc.frames_of("scaled_block", H, W, T, seed)}[kind]()


def _imbs_event(kind, part, T, H, W, seed, lead):
    """T frames of an imbs_numpy.clip whose scene changes at 1 / `part` of its length, cut so that the change falls on frame `lead`."""
    E = max(lead, T - lead)
    return im.clip(kind, part * E, H, W, seed)[E - lead:E - lead + T]


def build_inputs(case):
    """[S][T][H][W][3] uint8 from the case's input recipes."""
    T, H, W = case["T"], case["H"], case["W"]
    out = []
    for r in case["inputs"]:
        f = np.asarray(_clip(r["kind"], T, H, W, r["seed"], r.get("quiet", 0)), np.uint8)
        if r["cut"]:  # a scene cut
            c = T // 2
            f = np.concatenate([f[:c], 255 - f[c:]])
        out.append(f)
    return np.ascontiguousarray(np.stack(out))


# ---- adapters ---------------------------------------------------------------------------------------------------------------------

def _bgs_params(algo, prefix, p, skip=()):
    q = capi.default_params(algo)
    for k, v in p.items():
        if k not in skip:
            setattr(q, prefix + k, v)
    return q


class Adapter:
    family = ""
    classes = {}            # class name -> bgs_algo
    has_bg = False
    tols = {}               # class name -> {plane: tolerance}
    fetch = {}              # plane -> dtype the engine holds it in, where that is not the restatement's
    kinds = ()
    cut = True
    reset_rate = 0.3        # chance per call that one stream is reset, in a case that has resets (the old table's)
    h_small, w_small, h_big, w_big = H_SMALL, W_SMALL, H_BIG, W_BIG
    step_of = {}            # class name -> (parameter, function, default): one smallest step of one parameter (the sensitivity test)

    def needle(self, name):
        """What a refusal's message must contain."""
        return name

    def bg_shape(self, H, W):
        return (H, W, 3)

    def draw_frames(self, rng, p):
        return int(rng.integers(4, 23))

    def draw_bad(self, rng, name, p):
        return None

    def refusal(self, name, p):
        return None

    def follow(self, name, cur, new):
        """The parameters a running stream uses after bgs_set_*params(new) while `cur` was in force: frozen by default."""
        return cur

    def normalise(self, name, planes):
        return planes

    def accept(self, stats):
        return True

    def make_engine(self, name, p, S):
        from tracking_amd import Engine
        return Engine(self.classes[name], params=self.params_struct(name, p), n_streams=S)

    def apply(self, eng, name, p):
        eng.set_params(self.params_struct(name, p))


# -- KDE

class _KdeRef:
    def __init__(self, p):
        self.k = kn.Kde(**p)

    def step(self, f):
        return self.k.process(f), None, None

    def switch(self, p):
        pass

    def planes(self):
        k = self.k
        if k.first:
            return {}
        out = {"samples": k.seq, "qtop": k.qtop}
        if k.fn > k.F:  # Estimation has run
            out["sd_bins"], out["acc"] = k.sd, k.acc
        return out


class Kde(Adapter):
    family, classes = "kde", {"KDE": capi.KDE}
    kinds = ("dp2_scene", "dp2_scene", "lb_noisy", "synth_random", "synth_surv")
    step_of = {"KDE": ("threshold", lambda v: v * 1.25, None)}  # a density threshold: steps on a logarithmic scale

    def draw_params(self, rng, name, H, W, T):
        sl = int(rng.choice([3, 4, 6, 8, 12]))
        return dict(frames_to_learn=int(rng.integers(1, max(2, min(T - 2, 7)))), sequence_length=sl, time_window=int(sl * rng.choice([1, 2, 3, 5]) + rng.integers(0, 2)),
                    sd_estimation=int(rng.integers(0, 2)), color_ratios=int(rng.integers(0, 2)), update_model=int(rng.integers(0, 2)),
                    threshold=float(rng.choice([10e-8, 1e-5, 1e-10, 1e-6])), alpha=float(rng.choice([0.3, 0.1])))

    def draw_bad(self, rng, name, p):
        k, v = [("sequence_length", 2), ("sequence_length", 256), ("frames_to_learn", 0), ("time_window", 0), ("time_window", 256 * p["sequence_length"])][int(rng.integers(0, 5))]
        return k, v

    def refusal(self, name, p):
        sl = p["sequence_length"]
        if not 3 <= sl <= 255 or p["frames_to_learn"] < 1 or p["time_window"] < 1 or p["time_window"] // sl > 255:
            return capi.ERR_INVALID
        return None

    def draw_switch(self, rng, name, p):  # everything but framesToLearn and the update flag is kept once the geometry is set
        return dict(p, threshold=1e-3, sequence_length=p["sequence_length"] + 1, alpha=0.2, color_ratios=1 - p["color_ratios"])

    def params_struct(self, name, p):
        return _bgs_params(capi.KDE, "kde_", p)

    def make_ref(self, name, p, H, W, stats):
        return _KdeRef(p)


# -- DPPratiMediod, DPTexture

class _PratiRef:
    def __init__(self, p):
        self.m = dn.Prati(**p)

    def step(self, f):
        return self.m.process(f), None, None

    def switch(self, p):
        pass

    def planes(self):
        if self.m.fn == 0:
            return {}
        return dict(self.m.planes(), count=np.array([self.m.cnt, self.m.pos], np.int64))


class Prati(Adapter):
    family, classes = "prati", {"DPPratiMediod": capi.DP_PRATI_MEDIOD}
    kinds = ("dp2_scene", "dp2_scene", "dp2_tie", "synth_random", "lb_noisy")
    step_of = {"DPPratiMediod": ("threshold", lambda v: v + 1, None)}

    def needle(self, name):
        return "PratiMediod"

    def draw_params(self, rng, name, H, W, T):
        return dict(threshold=int(rng.choice([0, 5, 10, 25, 30, 60])), sampling_rate=int(rng.choice([1, 2, 3, 5])),
                    history_size=int(rng.choice([1, 2, 3, 4, 6, 16, 64], p=[.2, .2, .2, .15, .15, .05, .05])))

    def draw_bad(self, rng, name, p):
        return [("sampling_rate", 0), ("history_size", 0), ("history_size", capi.PRATI_MAX_HISTORY + 1), ("threshold", -1)][int(rng.integers(0, 4))]

    def refusal(self, name, p):
        if p["sampling_rate"] == 0 or not 1 <= p["history_size"] <= capi.PRATI_MAX_HISTORY or p["threshold"] < 0:
            return capi.ERR_UNSUPPORTED
        return None

    def draw_switch(self, rng, name, p):  # Initalize copied the parameters once
        return dict(threshold=p["threshold"] + 30, sampling_rate=p["sampling_rate"] % 5 + 1, history_size=p["history_size"] % 7 + 1)

    def params_struct(self, name, p):
        q = capi.default_params(capi.DP_PRATI_MEDIOD)
        q.dp_threshold, q.dp_sampling_rate, q.dp_history_size = float(p["threshold"]), p["sampling_rate"], p["history_size"]
        return q

    def make_ref(self, name, p, H, W, stats):
        return _PratiRef(p)


class _TextureRef:
    def __init__(self, hysteresis):
        self.m, self.h = dn.Texture(), hysteresis

    def step(self, f):
        keep, dn.HYSTERSIS = dn.HYSTERSIS, self.h
        try:
            return self.m.process(f), None, None
        finally:
            dn.HYSTERSIS = keep

    def switch(self, p):
        pass

    def planes(self):
        return {"hist": self.m.hist_plane()} if self.m.fn else {}


class Texture(Adapter):
    """No parameter of its own: nothing to refuse; the `switch` sets dp_* fields it never reads."""
    family, classes = "texture", {"DPTexture": capi.DP_TEXTURE}
    kinds = ("lb_noisy", "lb_noisy", "lb_noisy", "dp2_texture", "dp2_scene")  # noisy_clip's box reaches the interior within a few frames
    # below the 15 x 15 neighbourhood, just at it, above it; most frames large enough for their interior to hold 5 % of the pixels
    h_small, w_small = [1, 15, 33, 33, 40, 40, 48, 48, 48], [3, 40, 40, 48, 64, 64, 70, 70, 70]
    h_big, w_big = [33, 48], [64, 97]  # the restatement is the slowest of all (15 us per pixel and frame): the fewest pixels
    step_of = {"DPTexture": ("hysteresis", lambda v: v + 1, dn.HYSTERSIS)}  # no parameter: the test steps the restatement's constant

    def draw_params(self, rng, name, H, W, T):
        return {}

    def draw_switch(self, rng, name, p):
        return dict(dp_threshold=60.0, dp_alpha=0.5)

    def params_struct(self, name, p):
        return _bgs_params(capi.DP_TEXTURE, "", p, skip=("hysteresis",))

    def make_ref(self, name, p, H, W, stats):
        return _TextureRef(p.get("hysteresis", dn.HYSTERSIS))


# -- the five lb/ models

class _LbRef:
    def __init__(self, cls, p):
        self.m = ln.LB(cls, **p)

    def step(self, f):
        fg, bg = self.m.process(f)
        return fg, bg, None

    def switch(self, p):
        self.m.set(**p)

    def planes(self):
        return self.m.planes() if self.m.fn else {}


class Lb(Adapter):
    family, has_bg = "lb", True
    classes = {ln.NAMES[c]: getattr(capi, a) for c, a in ((25, "LB_SIMPLE_GAUSSIAN"), (26, "LB_FUZZY_GAUSSIAN"), (27, "LB_MOG"), (28, "LB_ADAPTIVE_SOM"), (29, "LB_FUZZY_ADAPTIVE_SOM"))}
    CLS = {v: k for k, v in ln.NAMES.items()}
    tols = {ln.NAMES[c]: t for c, t in ln.FUZZY_PLANE_TOL.items()}
    kinds = ("lb_noisy", "lb_modes", "lb_modes", "lb_tie", "synth_random")
    step_of = {n: ("sensitivity", lambda v: v + 1, None) for n in ln.NAMES.values()}

    def draw_params(self, rng, name, H, W, T):
        cls, p = self.CLS[name], {}
        lo_hi = dict(sensitivity=(20, 160), bg_threshold=(100, 240) if cls == 26 else (30, 250), learning_rate=(10, 256), noise_variance=(1, 256),
                     training_sensitivity=(100, 256), training_learning_rate=(100, 256), training_steps=(1, 30))
        for k in ln.DEFAULTS[cls]:
            p[k] = int(rng.integers(*lo_hi[k]))
        if rng.random() < 0.15:  # an end of the accepted range
            k = sorted(p)[int(rng.integers(0, len(p)))]
            p[k] = int(rng.choice([0, 255]))
            if self.refusal(name, p) is not None:
                p[k] = 254 if p[k] == 255 else 1
        return p

    def draw_bad(self, rng, name, p):
        cls = self.CLS[name]
        bad = [(k, v) for k in ln.DEFAULTS[cls] for v in (-1, 256, 300)]
        bad += [("noise_variance", 0)] * 3 if cls in (25, 26, 27) else [("training_steps", 0)] * 3
        if cls == 27:
            bad += [("bg_threshold", 255)] * 3
        return bad[int(rng.integers(0, len(bad)))]

    def refusal(self, name, p):  # DESIGN.md §5.5, "Decided and refused"
        cls = self.CLS[name]
        if any(not 0 <= v <= 255 for v in p.values()):
            return capi.ERR_UNSUPPORTED
        if cls in (25, 26, 27) and p["noise_variance"] == 0 or cls == 27 and p["bg_threshold"] == 255 or cls in (28, 29) and p["training_steps"] == 0:
            return capi.ERR_UNSUPPORTED
        return None

    def draw_switch(self, rng, name, p):  # setBGModelParameter runs every frame: every value is live
        return self.draw_params(rng, name, 0, 0, 0)

    def follow(self, name, cur, new):
        return new

    def params_struct(self, name, p):
        return _bgs_params(self.classes[name], "lb_", p)

    def make_ref(self, name, p, H, W, stats):
        return _LbRef(self.CLS[name], p)


# -- VuMeter

class _VuRef:
    def __init__(self, p):
        self.m = vn.VuMeter(**p)

    def step(self, f):
        fg, bg = self.m.process(f)
        return fg, bg, None

    def switch(self, p):
        self.m.enable_filter = p["enable_filter"]

    def planes(self):
        md = self.m.model
        if md.hist is None:
            return {}
        return {"hist": md.hist.reshape(md.bin_count, -1), "count": np.array([md.count], np.int64), "background": self.m.background.reshape(-1)}


class VuMeter(Adapter):
    """SetBinSize / SetAlpha / SetThreshold replace out-of-range values instead of refusing them: nothing to refuse;
    the out-of-range values are drawn as ordinary ones and the restatement applies the same setters."""
    family, classes, has_bg = "vumeter", {"VuMeter": capi.VUMETER}, True
    kinds = ("vu_box", "vu_box", "vu_leave", "lb_noisy", "synth_surv")
    h_small = [1, 4, 7, 16, 33, 64]  # 4 rows: below the 5 x 5 median
    step_of = {"VuMeter": ("bin_size", lambda v: v + 1, None)}

    def bg_shape(self, H, W):
        return (H, W)

    def draw_params(self, rng, name, H, W, T):
        # a bin that is hit k times in a row holds 1 - alpha^k: a pixel turns background after ln(1 - threshold) / ln(alpha) frames.
        # Most pairs put that between 1 and 10 frames; the others (never / at once) and the values the setters replace come rarely.
        pairs = [(0.995, 0.03)] * 3 + [(0.99, 0.03), (0.99, 0.1), (0.98, 0.1), (0.98, 0.03), (0.9, 0.3), (0.8, 0.3), (0.5, 0.03), (0.49, 0.3), (1.0, 0.0), (0.0, 1.5), (0.995, 0.3)]
        alpha, threshold = pairs[int(rng.integers(0, len(pairs)))]
        return dict(bin_size=int(rng.choice([8, 8, 8, 3, 7, 16, 64, 100, 0, 255, 300])), alpha=alpha, threshold=threshold, enable_filter=int(rng.integers(0, 2)))

    def draw_switch(self, rng, name, p):  # enableFilter is re-read every frame; the setters ran once
        return dict(bin_size=p["bin_size"] + 5, alpha=0.7, threshold=0.2, enable_filter=1 - p["enable_filter"])

    def follow(self, name, cur, new):
        return dict(cur, enable_filter=new["enable_filter"])

    def params_struct(self, name, p):
        return _bgs_params(capi.VUMETER, "vu_", p)

    def make_ref(self, name, p, H, W, stats):
        return _VuRef(p)


# -- the fuzzy integrals

class _FuzzyRef:
    def __init__(self, kind, p):
        self.m = fz.Fuzzy(kind, **p)
        self.detected = False

    def step(self, f):
        fg, bg = self.m.process(f)
        self.detected = fg is not None
        return fg, bg, None

    def switch(self, p):
        self.m.p.update(p)

    def planes(self):
        if self.m.bg is None:
            return {}
        out = {"background": self.m.bg, "count": np.array([self.m.frame_number], np.int64)}
        if self.detected:
            out["integral"] = self.m.integral
        return out


class Fuzzy(Adapter):
    family, has_bg = "fuzzy", True
    classes = {"FuzzySugenoIntegral": capi.FUZZY_SUGENO, "FuzzyChoquetIntegral": capi.FUZZY_CHOQUET}
    KIND = {"FuzzySugenoIntegral": fz.SUGENO, "FuzzyChoquetIntegral": fz.CHOQUET}
    FIELDS = dict(ftl="frames_to_learn", alphaLearn="alpha_learn", alphaUpdate="alpha_update", option="option", smooth="smooth", threshold="threshold", color_space="color_space")
    kinds = ("lb_noisy", "dp2_scene", "lb_modes", "t2f_scene", "synth_random", "synth_surv")
    h_small = [2, 3, 7, 16, 33, 64]  # frames lower than 2 rows are refused; 2 and 3 rows lie below the 3 x 3 LBP and the 3 x 3 median
    step_of = {n: ("threshold", lambda v: v + 2.0 ** -8, None) for n in classes}

    def draw_params(self, rng, name, H, W, T):
        return dict(ftl=int(rng.integers(0, max(1, min(T - 3, 5)))), alphaLearn=float(rng.choice([0.1, 0.3, 0.5])), alphaUpdate=float(rng.choice([0.01, 0.05, 0.2])),
                    option=int(rng.integers(1, 3)), smooth=int(rng.integers(0, 2)), threshold=float(rng.choice([0.67, 0.5, 0.8, 0.9])))

    def draw_bad(self, rng, name, p):
        return [("color_space", 2), ("color_space", 3), ("color_space", 4), ("color_space", 0), ("option", 0), ("option", 3), ("ftl", -1)][int(rng.integers(0, 7))]

    def refusal(self, name, p):  # DESIGN.md §5.7; in the order the engine checks
        if p.get("color_space", 1) != 1 or p["option"] not in (1, 2):
            return capi.ERR_UNSUPPORTED
        return capi.ERR_INVALID if p["ftl"] < 0 else None

    def draw_switch(self, rng, name, p):  # loadConfig runs every frame: all values act from the next frame on
        q = self.draw_params(rng, name, 0, 0, 8)
        if rng.random() < 0.6:
            q["ftl"] = p["ftl"]  # else: lowering it changes nothing for a detecting stream, raising it sends it back to learning
        return q

    def follow(self, name, cur, new):
        return new

    def make_engine(self, name, p, S):
        from tracking_amd import Engine
        eng = Engine(self.classes[name], n_streams=S)
        try:
            self.apply(eng, name, p)
        except capi.BgsError:
            eng.close()
            raise
        return eng

    def apply(self, eng, name, p):
        eng.set_fuzzy_params(**{self.FIELDS[k]: v for k, v in p.items()})

    def make_ref(self, name, p, H, W, stats):
        return _FuzzyRef(self.KIND[name], {k: v for k, v in p.items() if k != "color_space"})


# -- T2FGMM_UM / T2FGMM_UV

class _T2fRef:
    def __init__(self, typ, p, H, W):
        self.m, self.shape, self.seen = tn.T2FGMM(typ, H * W, **p), (H, W), 0

    def step(self, f):
        self.seen += 1
        return self.m.step(f).reshape(self.shape), None, None

    def switch(self, p):
        pass

    def planes(self):
        return {"nmodes": self.m.count, "modes": self.m.planes()} if self.seen else {}


class T2f(Adapter):
    family, classes = "t2f", {"T2FGMM_UM": capi.T2FGMM_UM, "T2FGMM_UV": capi.T2FGMM_UV}
    kinds = ("t2f_scene", "t2f_scene", "t2f_corners", "dp2_scene", "lb_modes")
    step_of = {"T2FGMM_UM": ("km", lambda v: v + 2.0 ** -20, None), "T2FGMM_UV": ("alpha", lambda v: float(np.nextafter(np.float32(v), np.float32(1))), None)}

    def draw_params(self, rng, name, H, W, T):
        return dict(threshold=float(rng.choice([9.0, 2.0, 4.0, 16.0])), alpha=float(rng.choice([0.001, 0.01, 0.01, 0.05, 0.2, 0.5])), km=float(rng.choice([1.5, 1.0, 2.0, 3.0])),
                    kv=float(np.float32(rng.choice([0.6, 0.3, 0.9]))), gaussians=int(rng.integers(1, 6)))

    def draw_bad(self, rng, name, p):
        bad = [("gaussians", 0), ("gaussians", 6), ("alpha", 1.0), ("alpha", -0.125), ("km", float("inf"))]
        if name == "T2FGMM_UV":
            bad += [("kv", 0.0)] * 2
        return bad[int(rng.integers(0, len(bad)))]

    def refusal(self, name, p):  # DESIGN.md §5.8, "Ids and parameters"
        f = np.float32
        with np.errstate(over="ignore"):
            finite = all(np.isfinite(f(p[k])) for k in ("threshold", "alpha", "km", "kv"))
        if not 1 <= p["gaussians"] <= 5 or not finite or not 0 <= f(p["alpha"]) < 1 or (name == "T2FGMM_UV" and f(p["kv"]) == 0):
            return capi.ERR_UNSUPPORTED
        return None

    def draw_switch(self, rng, name, p):  # taken when the geometry is set; a later call succeeds and changes nothing
        return dict(threshold=p["threshold"] + 5, alpha=0.3, km=p["km"] + 1, kv=0.5, gaussians=p["gaussians"] % 5 + 1)

    def normalise(self, name, planes):
        if "modes" not in planes:
            return planes
        cnt, modes = planes["nmodes"], planes["modes"]
        K = modes.shape[0] // tn.FIELDS
        below = tn.below_count(None, cnt, K).reshape(modes.shape)  # only the floats below a pixel's count are defined
        return {"nmodes": cnt, "modes": np.where(below, modes.view(np.uint32), 0)}

    def make_engine(self, name, p, S):
        from tracking_amd import Engine
        eng = Engine(self.classes[name], n_streams=S)
        try:
            self.apply(eng, name, p)
        except capi.BgsError:
            eng.close()
            raise
        return eng

    def apply(self, eng, name, p):
        eng.set_t2f_params(**p)

    def make_ref(self, name, p, H, W, stats):
        return _T2fRef(tn.TYPES.index(name[-2:].lower()), p, H, W)


# -- DPEigenbackground

class _EigenRef:
    def __init__(self, p, H, W, stats):
        self.p, self.m, self.shape, self.stats = p, en.Eigenbackground(p, H * W), (H, W), stats

    def step(self, f):
        m = self.m
        built = m.t >= m.H
        mask = m.step(f).reshape(self.shape)
        if not built:
            return mask, None, None
        if m.t == m.H + 1:  # the frame that built the model
            lam, M = m.lam, m.M
            gap = 0.0 if lam[M - 1] <= 1e-9 * lam[0] else (np.inf if M >= m.H or lam[M] <= 1e-9 * lam[0] else lam[M - 1] / lam[M])
            self.stats.setdefault("gaps", []).append(float(gap))
        near = en.band(self.p, f, m.result.astype(np.float64))
        self.stats["band"] = self.stats.get("band", 0) + int(near.sum())
        self.stats["detected"] = self.stats.get("detected", 0) + near.size
        return mask, None, near.reshape(self.shape)

    def switch(self, p):
        pass

    def planes(self):
        m = self.m
        if m.result is None:
            return {}
        S = m.history.astype(np.int64).sum(0)
        return {"history": m.history, "avg": S.astype(np.float32) / np.float32(m.H), "result": m.result.astype(np.float64)}


class Eigen(Adapter):
    family, classes = "eigen", {"DPEigenbackground": capi.DP_EIGENBACKGROUND}
    tols = {"DPEigenbackground": {"result": en.TOL_RESULT}}
    fetch = {"result": np.float32}
    kinds, cut = ("eigen_pca",), False
    reset_rate = 0.08  # a stream detects only after history_size frames in a row
    step_of = {"DPEigenbackground": ("threshold", lambda v: v + 1, None)}

    def draw_params(self, rng, name, H, W, T):
        hs = int(rng.integers(2, 17))
        top = max(1, min(hs - 1, 12, H * W * 3 // 2))  # pca_clip has 12 patterns: below them the spectrum is noise without a gap
        return dict(threshold=int(rng.choice([225, 225, 100, 400, 25])), history_size=hs, embedded_dim=int(rng.integers(1, top + 1)))

    def draw_frames(self, rng, p):  # at least 4 detecting frames
        hs = p["history_size"]
        return int(rng.integers(hs + 4, max(hs + 5, 23)))

    def draw_bad(self, rng, name, p):
        return [("history_size", 1), ("history_size", capi.EIGEN_MAX_HISTORY + 1), ("embedded_dim", 0), ("embedded_dim", p["history_size"])][int(rng.integers(0, 4))]

    def refusal(self, name, p):  # DESIGN.md §5.9, "Ids, parameters, refusals"
        if not 2 <= p["history_size"] <= capi.EIGEN_MAX_HISTORY or not 1 <= p["embedded_dim"] <= p["history_size"] - 1:
            return capi.ERR_UNSUPPORTED
        return None

    def draw_switch(self, rng, name, p):  # taken when the geometry is set
        return dict(threshold=p["threshold"] + 100, history_size=p["history_size"] % 9 + 2, embedded_dim=1)

    def accept(self, stats):
        """Parity is claimed for well-conditioned subspaces only, and the band may not swallow the comparison."""
        return bool(stats.get("gaps")) and all(g >= en.EIGENGAP for g in stats["gaps"]) and stats["band"] <= en.BAND_SHARE * stats["detected"]

    def make_engine(self, name, p, S):
        from tracking_amd import Engine
        eng = Engine(self.classes[name], n_streams=S)
        try:
            self.apply(eng, name, p)
        except capi.BgsError:
            eng.close()
            raise
        return eng

    def apply(self, eng, name, p):
        eng.set_eigen_params(**p)

    def make_ref(self, name, p, H, W, stats):
        return _EigenRef(p, H, W, stats)


# -- IndependentMultimodalBGS

class _ImbsRef:
    def __init__(self, p, H, W, stats):
        def area_filter(plane, min_area, _):
            out = im.area_filter_follower(plane, min_area)
            stats["filtered"] = stats.get("filtered", 0) + int(out.sum() < plane.sum())  # frames of which the filter removed something
            return out
        self.m, self.stats = im.Model(p, H, W, area_filter), stats

    def step(self, f):
        fg, bg = self.m.apply(f)
        for v in (80, 180):
            self.stats[v] = self.stats.get(v, 0) + int((fg == v).sum())
        return fg, bg, None

    def switch(self, p):
        pass

    def planes(self):
        return dict(self.m.planes(), control=self.m.control())


class Imbs(Adapter):
    """The contract is the restatement with the contour follower as its area filter.  Every frame delivers a mask
    and a background (zero images until the first model).  An inverted clip would leave the palette imbs_numpy.clip keeps to: no cut."""
    family, classes, has_bg, cut = "imbs", {im.CLASS_NAME: capi.IMBS}, True, False
    kinds = ("imbs_box", "imbs_box", "imbs_persist", "imbs_shadow", "imbs_holes", "imbs_sudden", "imbs_inject", "imbs_inject", "imbs_inject")
    reset_rate = 0.08  # a stream detects only after its first build
    # one row, the smallest frame with an interior, ragged, whole words; below 3 x 3 the filter leaves nothing, so most frames are larger
    h_small, w_small = [1, 3, 7, 16, 16, 33, 33], [3, 5, 37, 37, 64, 70, 70]
    h_big, w_big = [33, 65], [64, 97, 131]                    # the follower costs about 2 s a clip at 65 x 131
    step_of = {im.CLASS_NAME: ("minArea", lambda v: v + 0.5, None)}  # areas are exact halves; fgThreshold + 1 goes unnoticed in the first six cases
    CLOCKS = ((10.0, 100), (30.0, 33), (10.0, 200), (25.0, 80))  # (fps, samplingPeriod): a sample on every frame (the first two) or on every second one

    @staticmethod
    def lead(p):
        """Frames before the first detecting one: numSamples - 1 samples, the build, at one or two frames a sample."""
        stride = 1 if p["fps"] <= 0 or 1000. / p["fps"] >= p["samplingPeriod"] else 2
        return stride * (min(max(int(p["numSamples"]), 2), 63) - 1) + 1

    def draw_params(self, rng, name, H, W, T):
        fps, sp = self.CLOCKS[int(rng.choice([0, 0, 1, 2, 3]))]
        return dict(fps=fps, samplingPeriod=sp, numSamples=int(rng.integers(3, 13)), minBinHeight=int(rng.integers(1, 4)), fgThreshold=int(rng.choice([15, 10, 25, 40])),
                    associationThreshold=int(rng.choice([5, 3, 8, 4])), minArea=float(rng.choice([0.0, 2.5, 4.0, 30.0])), persistencePeriod=int(rng.choice([150, 300, 10000])),
                    alpha=float(rng.choice([0.65, 0.5, 0.8])), beta=float(rng.choice([1.15, 1.3, 1.0])), tau_s=int(rng.choice([60, 30, 255])), tau_h=int(rng.choice([40, 20, 0])),
                    morphologicalFiltering=int(rng.random() < 0.2))

    def draw_frames(self, rng, p):  # at least numSamples + 6: five or more detecting frames, and a second build where numSamples is small
        return self.lead(p) + int(rng.integers(6, 14))

    def draw_bad(self, rng, name, p):
        return [("numSamples", 1), ("numSamples", 64), ("minBinHeight", 0), ("minBinHeight", p["numSamples"] + 1), ("tau_s", 256), ("fps", 0.0)][int(rng.integers(0, 6))]

    def refusal(self, name, p):  # DESIGN.md §5.10, "Ids, parameters, refusals"
        f = np.float32
        if not (p["fps"] > 0 and np.isfinite(p["fps"])) or p["minBinHeight"] == 0 or not 2 <= p["numSamples"] <= capi.IMBS_MAX_SAMPLES or p["numSamples"] // p["minBinHeight"] == 0:
            return capi.ERR_UNSUPPORTED
        if not (0 <= p["tau_s"] <= 255 and 0 <= p["tau_h"] <= 255) or not all(np.isfinite(f(p[k])) for k in ("alpha", "beta")) or not np.isfinite(p["minArea"]):
            return capi.ERR_UNSUPPORTED
        return None

    def draw_switch(self, rng, name, p):  # taken when the geometry is set: a later call succeeds and changes nothing
        q = self.draw_params(rng, name, 0, 0, 0)
        return dict(q, fgThreshold=p["fgThreshold"] + 7, minArea=p["minArea"] + 3.0, numSamples=p["numSamples"] % 10 + 3)

    def make_engine(self, name, p, S):
        from tracking_amd import Engine
        eng = Engine(self.classes[name], n_streams=S)
        try:
            self.apply(eng, name, p)
        except capi.BgsError:
            eng.close()
            raise
        return eng

    def apply(self, eng, name, p):
        eng.set_imbs_params(**p)

    def make_ref(self, name, p, H, W, stats):
        return _ImbsRef(p, H, W, stats)


# -- MultiLayerBGS

_ml_sine = []


def _ml_min_sine_bits():
    """m_fMinNoisedAngleSine as the reference's own constructor computed it: the committed fixture's bits (all 17 cases hold the same)."""
    if not _ml_sine:
        _ml_sine.append(int(ml.load()["defaults"]["consts"][0]))
    return _ml_sine[0]


class _MultiLayerRef:
    def __init__(self, p, H, W, stats):
        self.m, self.stats = ml.Model(p, H, W, _ml_min_sine_bits()), stats

    def step(self, f):
        before = dict(self.m.counts)
        fg, bg = self.m.apply(f)
        for k, v in self.m.counts.items():  # the branch counters, summed over the case's streams
            self.stats[k] = self.stats.get(k, 0) + v - before[k]
        return fg, bg, None  # every frame delivers both; a stream's first mask is the reference's zero mask

    def switch(self, p):
        pass

    def planes(self):
        order, modes, dist = self.m.state()
        return {"order": order, "modes": modes, "dist": dist}


class MultiLayer(Adapter):
    """Everything is compared as raw bits: no tolerance, no redraw.  Parameters are frozen when the geometry is
    set, so a switch must change nothing, and a stream reset after one still runs the old values.  An inverted clip is an ordinary
    input."""
    family, classes, has_bg, cut = "multilayer", {ml.CLASS_NAME: capi.MULTILAYER}, True, True
    # static_block's 8 x 8 block is under 1 % of a big frame: scripted, dark and the block that scales with the frame come more often
    kinds = ("ml_scripted", "ml_scripted", "ml_scripted", "ml_dark", "ml_dark", "ml_scaled", "ml_scaled", "ml_scaled", "ml_block")
    # 1 x 1, one row, one column, 2 x 5, frames inside the largest halo (8) one or both ways, the smoothing tile's edges (32 x 8) from
    # both sides, ragged 37 x 53, whole words 16 x 64
    h_small, w_small = [1, 2, 7, 8, 9, 16, 33, 37], [1, 3, 5, 31, 32, 33, 37, 53, 64, 70, 33, 32, 31]
    h_big, w_big = [33, 65, 97, 130], [64, 97, 131, 261]
    # the mode learn rate of a stream in LEARN status, one float32 further (robust_LBP_constant 3 -> 4 lies under the MAX(., 5) clamp)
    step_of = {ml.CLASS_NAME: ("learn_mode_learn_rate_per_second", lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf))), None)}
    FLOATS = [k for k in ml.FIELDS if k not in ml.INT_FIELDS]

    def draw_params(self, rng, name, H, W, T):
        c = lambda *v: v[int(rng.integers(0, len(v)))]
        h = int(rng.integers(-1, 9))
        sigma = c(3.0, 0.5, 1.0, 5.0, 0.0) if h < 0 else c(3.0, 0.5, 1.0, 5.0)
        fast = rng.random() < 0.7  # with slow rates a short clip never creates a layer
        p = dict(max_mode_num=int(rng.integers(1, 6)), weight_updating_constant=c(0.0, 0.0, 5.0, 1.0), texture_weight=c(0.5, 0.3, 1.0, 0.0, -1.0),
                 bg_mode_percent=c(0.6, 0.3, 0.9), pattern_neig_half_size=h, pattern_neig_gaus_sigma=sigma, bg_prob_threshold=c(0.2, 0.1, 0.4),
                 bg_prob_updating_threshold=c(0.2, 0.1, 0.35), robust_LBP_constant=c(3, 5, 6, 12), min_noised_angle=c(ml.DEFAULTS["min_noised_angle"], 0.05, 0.5),
                 shadow_rate=c(0.6, 0.4, 1.0), highlight_rate=c(1.2, 1.0, 2.0), frame_duration=c(0.1, 0.1, 0.1, 0.04),
                 learn_mode_learn_rate_per_second=c(5.0, 2.0) if fast else c(5.0, 0.5, 2.0), learn_weight_learn_rate_per_second=c(5.0, 5.0, 5.0, 2.0) if fast else c(5.0, 0.5, 2.0),
                 learn_init_mode_weight=c(0.05, 0.2))
        for k, v in (("detect_mode_learn_rate_per_second", (0.5, 2.0)), ("detect_weight_learn_rate_per_second", (0.5, 5.0)), ("detect_init_mode_weight", (0.05, 0.2))):
            p[k] = c(*v) if rng.random() < 1 / 3 else ml.DEFAULTS[k]
        flags = int(rng.integers(0, 8))
        p.update(status=flags & 1, disable_detect_mode=flags >> 1 & 1, disable_learning=flags >> 2 & 1)
        p["detect_after"] = [0, 0, 3, max(T, 8) // 2][int(rng.integers(0, 4))]  # draw_frames makes the last one T // 2
        return {k: p[k] for k in ml.FIELDS}

    def draw_frames(self, rng, p):
        """8-30 frames (scripted changes its scene at frame 6; a layer that is not seen again is removed 14 frames later); a
        detect_after above 3 falls on T // 2 of a clip of 8-22 frames."""
        da, T = p["detect_after"], int(rng.integers(8, 31))
        return T if da <= 3 else 2 * da + int(rng.integers(0, 2)) * (da < 11)

    def draw_bad(self, rng, name, p):
        bad = [("max_mode_num", 0), ("max_mode_num", 6), ("pattern_neig_half_size", 9), ("texture_weight", float("nan")), ("frame_duration", float("inf"))]
        if p["pattern_neig_half_size"] >= 0:  # without smoothing the sigma is never read and not refused
            bad += [("pattern_neig_gaus_sigma", 0.0), ("pattern_neig_gaus_sigma", -1.0)]
        return bad[int(rng.integers(0, len(bad)))]

    def refusal(self, name, p):  # ml_check, engine_multilayer.h
        with np.errstate(over="ignore"):
            finite = all(np.isfinite(np.float32(p[k])) for k in self.FLOATS)
        h = p["pattern_neig_half_size"]
        if not finite or not 1 <= p["max_mode_num"] <= ml.K or h > capi.MULTILAYER_MAX_HALF_SIZE or (h >= 0 and not p["pattern_neig_gaus_sigma"] > 0):
            return capi.ERR_UNSUPPORTED
        return None

    def draw_switch(self, rng, name, p):  # a valid draw that an engine which wrongly took it would show
        q = self.draw_params(rng, name, 0, 0, 8)
        q.update(max_mode_num=p["max_mode_num"] % ml.K + 1, bg_prob_threshold=p["bg_prob_threshold"] + 0.15, pattern_neig_half_size=(p["pattern_neig_half_size"] + 2) % 9)
        if not q["pattern_neig_gaus_sigma"] > 0:
            q["pattern_neig_gaus_sigma"] = 3.0
        return q

    def make_engine(self, name, p, S):
        from tracking_amd import Engine
        eng = Engine(self.classes[name], n_streams=S)
        try:
            self.apply(eng, name, p)
        except capi.BgsError:
            eng.close()
            raise
        return eng

    def apply(self, eng, name, p):
        eng.set_multilayer_params(**p)

    def make_ref(self, name, p, H, W, stats):
        return _MultiLayerRef(p, H, W, stats)


ADAPTERS = [Kde(), Prati(), Texture(), Lb(), VuMeter(), Fuzzy(), T2f(), Eigen(), Imbs(), MultiLayer()]
BY_CLASS = {name: ad for ad in ADAPTERS for name in ad.classes}
MODELS = sorted(BY_CLASS)
FAMILIES = {ad.family: sorted(ad.classes) for ad in ADAPTERS}
MAX_REDRAWS = 8


# ---- a case: drawn without a GPU, restated without a GPU ----------------------------------------------------------------------------

def _draw_once(rng, seed, classes, big, attempt):
    name = str(rng.choice(sorted(classes)))
    ad = BY_CLASS[name]
    H, W = int(rng.choice(ad.h_big if big else ad.h_small)), int(rng.choice(ad.w_big if big else ad.w_small))
    S = int(rng.integers(1, 4))
    T0 = int(rng.integers(4, 23))
    p = ad.draw_params(rng, name, H, W, T0)
    T = T0 if type(ad).draw_frames is Adapter.draw_frames else ad.draw_frames(rng, p)
    bad = None
    if rng.random() < 0.12:
        bad = ad.draw_bad(rng, name, p)
        if bad is not None:
            p = dict(p, **{bad[0]: bad[1]})
    inputs = []
    for s in range(S):
        r = dict(kind=str(rng.choice(ad.kinds)), seed=seed * 7 + s + 1000003 * attempt, cut=bool(ad.cut and rng.random() < 0.3))
        if r["kind"] == "eigen_pca":
            r["quiet"] = p["history_size"] + 2  # the box stays out of a fresh stream's history
        elif r["kind"].startswith("imbs_"):
            r["quiet"] = ad.lead(p)  # what a clip shows starts where a fresh stream detects
        inputs.append(r)
    mode = str(rng.choice(MODES))
    resets = bool(rng.random() < 0.35)
    switch = None
    if rng.random() < 0.4:
        switch = dict(t=int(rng.integers(1, T)), params=ad.draw_switch(rng, name, p))
    steps, t = [], 0
    while t < T:
        st = dict(t=t, n=1, resets=[])
        if resets and t > 0 and rng.random() < ad.reset_rate:
            st["resets"].append(int(rng.integers(0, S)))
        m = mode if mode != "mixed" else str(rng.choice(MODES[:5]))
        if m == "clip":
            st["n"] = int(min(T - t, rng.integers(1, 12)))
            if switch and t < switch["t"]:
                st["n"] = min(st["n"], switch["t"] - t)  # a call ends where the parameters change
        if m == "ranges":
            st["split"] = int(rng.integers(1, S)) if S > 1 else 1
        st["m"] = m
        steps.append(st)
        t += st["n"]
    return dict(table="models", seed=int(seed), big=bool(big), redraws=attempt, family=ad.family, name=name, H=H, W=W, S=S, T=T, params=p,
                bad=None if bad is None else bad[0], inputs=inputs, mode=mode, steps=steps, switch=switch)


def draw_model_case(rng, seed, classes, big):
    """One case of the `models` table.  Pure: numpy and the restatements only.  A family that claims parity on part of its inputs only
    (Eigen: a model gets built, its eigengap is at least EIGENGAP, at most BAND_SHARE of the pixel-frames lie near a threshold)
    restates the draw and draws again from the seed's next generator, (seed, 1), (seed, 2), ..., until the draw qualifies: a case is
    never dropped."""
    for attempt in range(MAX_REDRAWS + 1):
        case = _draw_once(rng if attempt == 0 else np.random.default_rng([seed, attempt]), seed, classes, big, attempt)
        ad = BY_CLASS[case["name"]]
        if type(ad).accept is Adapter.accept or ad.refusal(case["name"], case["params"]) is not None:
            return case
        if ad.accept(reference_run(case)[2]):
            return case
    raise AssertionError("seed %d: no qualifying draw in %d attempts" % (seed, MAX_REDRAWS + 1))


def reference_run(case, frames=None, params=None):
    """The restatement's side of a case: outs[s][t] = (mask or None, background or None, ignore or None), the restatement of every
    stream after the last frame, and what the adapter collected on the way.  `params` replaces the case's own (the sensitivity test)."""
    ad, name, H, W = BY_CLASS[case["name"]], case["name"], case["H"], case["W"]
    frames = build_inputs(case) if frames is None else frames
    stats = {}
    cur = dict(case["params"] if params is None else params)
    refs = [ad.make_ref(name, cur, H, W, stats) for _ in range(case["S"])]
    outs = [[None] * case["T"] for _ in range(case["S"])]
    sw = case["switch"]
    for st in case["steps"]:
        if sw and st["t"] == sw["t"]:
            cur = ad.follow(name, cur, sw["params"])
            for r in refs:
                r.switch(cur)
        for r in st["resets"]:
            refs[r] = ad.make_ref(name, cur, H, W, stats)
        for s in range(case["S"]):
            for t in range(st["t"], st["t"] + st["n"]):
                outs[s][t] = refs[s].step(frames[s][t])
    return outs, refs, stats


def describe(case):
    return "%s %dx%d x%d streams, %d frames, %s%s%s %s" % (case["name"], case["W"], case["H"], case["S"], case["T"], case["mode"],
                                                           " +resets" if any(st["resets"] for st in case["steps"]) else "",
                                                           " +switch@%d" % case["switch"]["t"] if case["switch"] else "", case["params"])


# ---- the fixed slices of the suite: (id, classes, big, first seed, cases) -----------------------------------------------------------
# One class per slice, so that the restatement's side of a slice stays near 3 s on the CPU; tests/test_fuzz_models_cpu.py holds every
# slice to the conditions a class needs (accepted cases, entry points, geometries, resets, switches, refusals, lively masks).

# The 14 classes of the first table keep the index, and with it the seeds, of their place in their sorted list; a class that joined
# later takes the next free index, whatever its place in the alphabet
LATE_JOINERS = {im.CLASS_NAME: 14, ml.CLASS_NAME: 15}


def _slices():
    out = []
    first14 = [n for n in MODELS if n not in LATE_JOINERS]
    assert len(first14) == 14 and sorted(LATE_JOINERS.values()) == list(range(14, len(MODELS)))
    for name in MODELS:
        k = LATE_JOINERS[name] if name in LATE_JOINERS else first14.index(name)
        fam = BY_CLASS[name].family
        small, small_parts, big, big_parts = SLICE_CASES.get(name, SLICE_CASES["*"])
        for size, is_big, first, count, parts in (("small", False, 700000 + 1000 * k, small, small_parts), ("big", True, 800000 + 1000 * k, big, big_parts)):
            cuts = [count * i // parts for i in range(parts + 1)]
            for i in range(parts):
                out.append(("%s-%s-%s-%d" % (fam, name, size, i), (name,), is_big, first + cuts[i], cuts[i + 1] - cuts[i]))
    return out


# class -> (small cases, slices they are cut into, big cases, slices they are cut into); cut where a restatement is slow
SLICE_CASES = {"*": (36, 1, 8, 1), "DPTexture": (28, 4, 6, 3), "LBAdaptiveSOM": (36, 2, 8, 2), "LBFuzzyAdaptiveSOM": (36, 2, 8, 4), "LBMixtureOfGaussians": (36, 1, 8, 2),
               "T2FGMM_UV": (36, 1, 8, 2), im.CLASS_NAME: (36, 1, 8, 4), ml.CLASS_NAME: (36, 1, 8, 2)}
SLICES = _slices()


def slices_of(name, big):
    return [s[0] for s in SLICES if s[1] == (name,) and s[2] == big]


def slice_cases(first, count, classes, big):
    return [draw_model_case(np.random.default_rng(seed), seed, classes, big) for seed in range(first, first + count)]
