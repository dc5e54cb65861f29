"""DPPratiMediodBGS / DPTextureBGS (BGS_DP_PRATI_MEDIOD, BGS_DP_TEXTURE; USTC_BGS types 14 and 16) on the MI355X: masks equal the
reference's own code (tests/golden/dp2_ref_*.npz: pinned), model planes and every multi-stream path equal the numpy restatement
(tests/dp2_numpy.py, pinned by the same fixtures)."""
import subprocess

import numpy as np
import pytest

import dp2_numpy as dn
from test_dp2_cpu import PRATI_CASES, TEXTURE_CASES, golden, masks_of, prati_kwargs
from tracking_amd import Engine, capi

from gpu_helpers import _torch

pytestmark = pytest.mark.gpu


def prati_params(threshold=30, sampling_rate=5, history_size=16):
    p = capi.default_params(capi.DP_PRATI_MEDIOD)
    p.dp_threshold, p.dp_sampling_rate, p.dp_history_size = float(threshold), sampling_rate, history_size
    return p


def make(algo, kw=None, n_streams=1):
    if algo == capi.DP_PRATI_MEDIOD:
        return Engine(algo, params=prati_params(**(kw or {})), n_streams=n_streams), (lambda **x: dn.Prati(**(kw or {}), **x))
    return Engine(algo, n_streams=n_streams), (lambda **x: dn.Texture(**x))


def prati_planes(eng, H, n, stream=0):
    return {"samples": eng.get_state("samples", (H, n, 3), np.uint8, stream), "dist": eng.get_state("dist", (H, n), np.uint16, stream),
            "median": eng.get_state("median", (n, 3), np.uint8, stream)}


@pytest.mark.parametrize("case", PRATI_CASES)
def test_prati_masks_equal_reference_fixture(case):
    r, p, frames = golden("prati", case)
    eng = Engine(capi.DP_PRATI_MEDIOD, params=prati_params(**prati_kwargs(p)))
    want = masks_of(r)
    for t, f in enumerate(frames):
        fg, bg = eng.process(f)
        assert bg is None
        assert np.array_equal(fg, want[t]), (case, t, int((fg != want[t]).sum()))
    if "samples" in r:
        n = frames.shape[1] * frames.shape[2]
        got = prati_planes(eng, p["history_size"], n)
        for name in ("samples", "dist", "median"):
            assert np.array_equal(got[name], r[name]), name
        assert tuple(eng.get_state("count", (2,), np.int64)) == tuple(int(v) for v in r["count"])
    eng.close()


@pytest.mark.parametrize("case", TEXTURE_CASES)
def test_texture_masks_equal_reference_fixture(case):
    r, p, frames = golden("texture", case)
    eng = Engine(capi.DP_TEXTURE)
    want = masks_of(r)
    for t, f in enumerate(frames):
        fg, bg = eng.process(f)
        assert bg is None
        assert np.array_equal(fg, want[t]), (case, t, int((fg != want[t]).sum()))
    if "hist_interior" in r:
        T, H, W = (int(v) for v in r["shape"])
        hist = eng.get_state("hist", (H, W, 3, 64), np.uint8)
        e = dn.EDGE
        assert np.array_equal(hist[e:H - e, e:W - e], r["hist_interior"])
        hist[e:H - e, e:W - e] = 0
        assert not hist.any()  # 0 outside the interior
    eng.close()


def test_prati_model_planes_follow_the_restatement():
    """History 6, rate 2 on a tie-heavy clip: every plane after every frame (filling, wrap, stale-slot medoids)."""
    kw = dict(threshold=20, sampling_rate=2, history_size=6)
    frames = dn.tie_clip(40, 13, 11, seed=21)
    eng, ref = Engine(capi.DP_PRATI_MEDIOD, params=prati_params(**kw)), dn.Prati(**kw)
    n = 13 * 11
    for t, f in enumerate(frames):
        fg, _ = eng.process(f)
        assert np.array_equal(fg, ref.process(f)), t
        got = prati_planes(eng, 6, n)
        for name, v in ref.planes().items():
            assert np.array_equal(got[name], v), (t, name)
        assert tuple(eng.get_state("count", (2,), np.int64)) == (ref.cnt, ref.pos), t
    eng.close()


def test_prati_hysteresis_at_the_border_and_around_isolated_high_pixels():
    """Median 100 everywhere; frame 1 (history 1, rate 1): an isolated high pixel pulls in its low 8-neighbours, a low pixel with no
    high neighbour stays background, a high pixel on the border stays background, and so does a low pixel next to it."""
    H, W = 12, 16
    base = np.full((H, W, 3), 100, np.uint8)
    f = base.copy()
    f[5, 5] = (100, 200, 100)          # high (100 > 60)
    f[4, 4] = f[6, 6] = (140, 100, 100)  # low (40 > 30), next to the high one
    f[4, 8] = (100, 100, 135)           # low, no high neighbour
    f[0, 10] = (0, 100, 100)            # high, on the border
    f[1, 10] = (100, 65, 100)           # low, next to the border one
    f[1, 11] = (100, 100, 100)
    eng, ref = Engine(capi.DP_PRATI_MEDIOD, params=prati_params(30, 1, 1)), dn.Prati(30, 1, 1)
    for x in (base, f):
        fg, _ = eng.process(x)
        want = ref.process(x)
        assert np.array_equal(fg, want)
    exp = np.zeros((H, W), np.uint8)
    exp[5, 5] = exp[4, 4] = exp[6, 6] = exp[1, 10] = 255
    assert np.array_equal(fg, exp)
    eng.close()


@pytest.mark.parametrize("H,W", [(40, 96), (96, 40), (45, 37), (30, 62)])
def test_texture_geometries_follow_the_restatement(H, W):
    """Landscape (gate reads past the image), portrait, and W % 4 != 0 (gate reads on row padding): the rule of DESIGN.md §5.4."""
    frames = dn.texture_clip(14, H, W, seed=H * 100 + W)
    eng, ref = Engine(capi.DP_TEXTURE), dn.Texture()
    for t, f in enumerate(frames):
        fg, _ = eng.process(f)
        want = ref.process(f)
        assert np.array_equal(fg, want), (H, W, t, int((fg != want).sum()))
    assert np.array_equal(eng.get_state("hist", (H * W, 3, 64), np.uint8), ref.hist_plane())
    eng.close()


@pytest.mark.parametrize("algo", [capi.DP_PRATI_MEDIOD, capi.DP_TEXTURE])
def test_small_frames_give_empty_masks(algo):
    for H, W in ((14, 14), (14, 40), (2, 2), (1, 5)):
        kw = dict(threshold=0, sampling_rate=1, history_size=1) if algo == capi.DP_PRATI_MEDIOD else None
        eng, mk = make(algo, kw)
        ref = mk()
        frames = np.random.default_rng(H * W).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
        for f in frames:
            fg, _ = eng.process(f)
            want = ref.process(f)
            assert np.array_equal(fg, want)
            if algo == capi.DP_TEXTURE or min(H, W) < 3:
                assert not fg.any(), (H, W)
        eng.close()


@pytest.mark.parametrize("algo", [capi.DP_PRATI_MEDIOD, capi.DP_TEXTURE])
def test_streams_of_different_ages_ranges_reset_and_ragged_bits(algo):
    """8 streams aged 0..7 frames in one batch call; then two ranges on two HIP streams; a reset mid-run; a 37x53 geometry whose
    packed masks straddle streams.  Every mask and packed word equals a per-stream restatement run."""
    torch = _torch()
    S, H, W, T = 8, 37, 53, 16
    kw = dict(threshold=25, sampling_rate=3, history_size=4) if algo == capi.DP_PRATI_MEDIOD else None
    clips = [dn.scene_clip(T + S, H, W, seed=40 + s, box=0.15) for s in range(S)]
    eng, mk = make(algo, kw, n_streams=S)
    eng.set_geometry(H, W, 3)
    refs = [mk() for _ in range(S)]
    pos = [0] * S

    def feed(s):
        want = refs[s].process(clips[s][pos[s]])
        pos[s] += 1
        return want

    for s in range(S):  # stream s has seen s frames
        for _ in range(s):
            d = torch.from_numpy(clips[s][pos[s]]).cuda().unsqueeze(0)
            eng.process_batch_device(d, None, None, None, first=s, count=1)
            feed(s)
    Wd = (H * W + 63) // 64
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for step in range(T):
        frames = np.stack([clips[s][pos[s]] for s in range(S)])
        d = torch.from_numpy(frames).cuda()
        d_fg = torch.full((S, H, W), 7, dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((S, Wd), dtype=torch.int64, device="cuda")
        if step == 9:
            eng.reset_stream(5)
            refs[5] = mk()
        if step % 2 == 0:
            eng.process_batch_device(d, d_fg, None, d_bits)
        else:  # two ranges on two HIP streams, each ordered after the upload
            torch.cuda.current_stream().synchronize()
            eng.process_batch_device(d[:3], d_fg[:3], None, d_bits[:3], hip_stream=s1.cuda_stream, first=0, count=3)
            eng.process_batch_device(d[3:], d_fg[3:], None, d_bits[3:], hip_stream=s2.cuda_stream, first=3, count=5)
            s1.synchronize(), s2.synchronize()
        torch.cuda.synchronize()
        fg, bits = d_fg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            want = feed(s)
            assert np.array_equal(fg[s], want), (step, s, int((fg[s] != want).sum()))
            packed = np.packbits(want.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
            wbits = np.zeros(Wd * 8, np.uint8)
            wbits[:len(packed)] = packed
            assert np.array_equal(bits[s], wbits.view(np.uint64)), (step, s)
            assert eng.stream_flags(s) & capi.FG_VALID
            assert eng.frames_seen(s) == refs[s].fn
    eng.close()


def test_prati_parameters_are_fixed_at_the_first_frame():
    frames = dn.scene_clip(30, 16, 20, seed=3)
    kw = dict(threshold=10, sampling_rate=2, history_size=4)
    eng, ref = Engine(capi.DP_PRATI_MEDIOD, params=prati_params(**kw)), dn.Prati(**kw)
    for t, f in enumerate(frames):
        if t == 5:
            eng.set_params(prati_params(60, 1, 9))  # ignored: Initalize copied the parameters once
        fg, _ = eng.process(f)
        assert np.array_equal(fg, ref.process(f)), t
    eng.close()


def frame_1080(t, seed, base, noise):
    """Cheap seeded 1080p frame: textured base + a rolled noise field + a moving box of vertical stripes (a texture of its own)."""
    f = base + np.roll(noise, (t * 7) % 97, axis=1)
    y, x = (t * 9) % 700, (t * 17) % 1400
    f[y:y + 300, x:x + 400] = np.where(np.arange(400) % 4 < 2, 230, 20)[None, :, None]
    return np.clip(f, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("algo", [capi.DP_PRATI_MEDIOD, capi.DP_TEXTURE])
def test_two_1080p_streams_equal_restatement_on_a_pixel_sample(algo):
    torch = _torch()
    S, H, W, T = 2, 1080, 1920, 90
    rng = np.random.default_rng(5)
    bases = [rng.integers(30, 220, (H, W, 3)).astype(np.int16) for _ in range(S)]
    noises = [rng.integers(-4, 5, (H, W, 3)).astype(np.int16) for _ in range(S)]
    edges = np.concatenate([np.arange(0, 96), W + np.arange(0, 96), 7 * W + np.arange(0, 96), H * W - 1 - np.arange(96)])
    sample = np.unique(np.concatenate([rng.integers(0, H * W, 1500), edges]))
    eng, mk = make(algo, None, n_streams=S)
    eng.set_geometry(H, W, 3)
    refs = [mk(pixels=sample) for _ in range(S)]
    Wd = H * W // 64
    checked = 0
    for t in range(T):
        frames = np.stack([frame_1080(t, s, bases[s], noises[s]) for s in range(S)])
        d = torch.from_numpy(frames).cuda()
        d_fg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((S, Wd), dtype=torch.int64, device="cuda")
        flags = eng.process_batch_device(d, d_fg, None, d_bits)
        torch.cuda.synchronize()
        assert flags & capi.FG_VALID
        fg, bits = d_fg.cpu().numpy().reshape(S, -1), d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            want = refs[s].process(frames[s]).reshape(-1)
            assert np.array_equal(fg[s][sample], want[sample]), (t, s, int((fg[s][sample] != want[sample]).sum()))
            assert np.array_equal(bits[s], np.packbits(fg[s] != 0, bitorder="little").view(np.uint64)), (t, s)
            checked += int((want[sample] != 0).sum())
    assert checked > 1000  # the sample saw foreground
    eng.close()


def test_demo_ustc_types_14_16_and_frame_processor_equal_fixture(tmp_path):
    """The host C++ layer: USTC_BGS(14) / (16) (tracker path) and FrameProcessor with enableDPPratiMediodBGS / enableDPTextureBGS,
    against the reference's own masks."""
    from test_gpu_01_host_cpp import HOST, DEMO, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    r, p, frames = golden("prati", "frames96")  # history 6, rate 1, threshold 20 (through DPPratiMediodBGS.xml)
    want_pm = masks_of(r)
    _, _, tframes = golden("texture", "crop48x80")
    want_tx = masks_of(golden("texture", "crop48x80")[0])
    for typ, cls, clip, want, xml in ((14, "DPPratiMediodBGS", frames, want_pm,
                                        "<threshold>20</threshold>\n<samplingRate>1</samplingRate>\n<historySize>6</historySize>\n"),
                                       (16, "DPTextureBGS", tframes, want_tx, "")):
        raw = str(tmp_path / ("%s.raw" % cls))
        clip.tofile(raw)
        n, rows, cols = clip.shape[:3]
        for mode in ("ustc", "fp"):
            wd = tmp_path / ("%s_%s" % (cls, mode))
            (wd / "config").mkdir(parents=True)
            if xml:
                (wd / "config" / ("%s.xml" % cls)).write_text('<?xml version="1.0"?>\n<opencv_storage>\n%s</opencv_storage>\n' % xml)
            if mode == "ustc":
                args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out"), str(typ)]
                out = wd / "out.ustc.raw"
            else:
                write_fp_config(str(wd / "config"), set())
                with open(str(wd / "config" / "FrameProcessor.xml")) as f:
                    text = f.read().replace("</opencv_storage>", "<enable%s>1</enable%s>\n</opencv_storage>" % (cls, cls))
                with open(str(wd / "config" / "FrameProcessor.xml"), "w") as f:
                    f.write(text)
                args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out")]
                out = wd / ("out.%s.raw" % cls)
            res = subprocess.run(args, cwd=str(wd), capture_output=True, text=True)
            assert res.returncode == 0, res.stdout + res.stderr
            got = np.fromfile(str(out), np.uint8).reshape(n, rows, cols)
            assert np.array_equal(got, want), (cls, mode, int((got != want).sum()))
            saved = (wd / "config" / ("%s.xml" % cls)).read_text()
            assert "<showOutput>1</showOutput>" in saved
            if typ == 14:
                assert "<historySize>6</historySize>" in saved and "<weight>5</weight>" in saved
