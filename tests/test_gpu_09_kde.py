"""KDE (BGS_KDE, USTC_BGS type 32) on the MI355X: masks equal the reference's own code (tests/golden/kde_ref*.npz: pinned),
model planes and every multi-stream path equal the numpy restatement (tests/kde_numpy.py, pinned by the same fixtures)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import kde_numpy as kn
from test_kde_cpu import CASES, golden_cases, kde_kwargs, masks_of
from tracking_amd import Engine, capi

from gpu_helpers import _torch

pytestmark = pytest.mark.gpu


def params(**kw):
    p = capi.default_params(capi.KDE)
    for k, v in kw.items():
        setattr(p, "kde_" + k, v)
    return p


def planes(eng, SL, n, C_, stream=0):
    return {"samples": eng.get_state("samples", (SL, n, C_), np.uint8, stream), "sd_bins": eng.get_state("sd_bins", (n, C_), np.uint8, stream),
            "qtop": eng.get_state("qtop", (n,), np.uint8, stream), "acc": eng.get_state("acc", (n,), np.uint32, stream)}


def scene(T, H, W, seed, fg_frac=0.1):
    """Static textured scene with +-3 sensor noise and a moving box covering about fg_frac of the frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(30, 200, (H, W, 3), dtype=np.int16)
    bh, bw = int(H * np.sqrt(fg_frac)), int(W * np.sqrt(fg_frac))
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        f = base + rng.integers(-3, 4, (H, W, 3), dtype=np.int16)
        y, x = (t * 3) % max(H - bh, 1), (t * 5) % max(W - bw, 1)
        f[y:y + bh, x:x + bw] = (230, 40, 90)
        out[t] = np.clip(f, 0, 255)
    return out


@pytest.mark.parametrize("case", CASES + ["long"])
def test_masks_equal_reference_fixture(case):
    r, p, frames = golden_cases()[case]
    eng = Engine(capi.KDE, params=params(**kde_kwargs(p)))
    want = masks_of(r)
    F = p["frames_to_learn"]
    for t, f in enumerate(frames):
        fg, bg = eng.process(f)
        assert bg is None
        if t < F:
            assert fg is None, t
        else:
            assert np.array_equal(fg, want[t - F]), (case, t, int((fg != want[t - F]).sum()))
    if case == "long":
        got = planes(eng, 50, 256, 3)
        for name in ("samples", "sd_bins", "qtop", "acc"):
            assert np.array_equal(got[name], r[name]), name
    eng.close()


def test_model_planes_follow_the_restatement(golden_frames):
    """SL 8, TW 40 (temporal length 5), 3 learning frames: planes after learning, after Estimation and after every update."""
    kw = dict(frames_to_learn=3, sequence_length=8, time_window=40)
    eng, ref = Engine(capi.KDE, params=params(**kw)), kn.Kde(**kw)
    n = golden_frames.shape[1] * golden_frames.shape[2]
    for t, f in enumerate(golden_frames):
        fg, _ = eng.process(f)
        want = ref.process(f)
        assert (fg is None) == (want is None) and (fg is None or np.array_equal(fg, want)), t
        got = planes(eng, 8, n, 3)
        assert np.array_equal(got["samples"], ref.seq) and np.array_equal(got["qtop"], ref.qtop), t
        if t >= 3:
            assert np.array_equal(got["sd_bins"], ref.sd) and np.array_equal(got["acc"], ref.acc), t
    eng.close()


def test_gray_and_channel_rejections(golden_gray):
    with pytest.raises(capi.BgsError) as ei:  # BGR2SnGnRn on a gray frame reads past it in the reference
        Engine(capi.KDE).process(golden_gray[0])
    assert ei.value.code == capi.ERR_UNSUPPORTED
    eng = Engine(capi.KDE)
    with pytest.raises(capi.BgsError) as ei:
        eng.set_geometry(8, 8, 2)
    assert ei.value.code == capi.ERR_UNSUPPORTED


def test_bgr2sngnrn_on_device_all_triples():
    """Every (b, g, r) byte triple through the learning launch: slot 0 of the samples equals BGR2SnGnRn."""
    img = np.arange(1 << 24, dtype=np.uint32).view(np.uint8).reshape(4096, 4096, 4)[..., :3].copy()
    eng = Engine(capi.KDE, params=params(frames_to_learn=1, sequence_length=3, time_window=3))
    assert eng.process(img) == (None, None)
    got = eng.get_state("samples", (3, 4096 * 4096, 3), np.uint8)[0]
    assert np.array_equal(got, kn.bgr2sngnrn(img.reshape(-1, 3)))
    eng.close()


def test_streams_of_different_ages_ranges_reset_and_ragged_bits():
    """8 streams aged 0..7 frames in one batch call; then two ranges on two HIP streams; a reset mid-run; a 37x53 geometry whose
    packed masks straddle streams.  Every mask and packed word equals a per-stream restatement run."""
    torch = _torch()
    S, H, W, T = 8, 37, 53, 16
    kw = dict(frames_to_learn=4, sequence_length=6, time_window=18)
    clips = [scene(T + S, H, W, seed=40 + s, fg_frac=0.15) for s in range(S)]
    eng = Engine(capi.KDE, params=params(**kw), n_streams=S)
    eng.set_geometry(H, W, 3)
    refs = [kn.Kde(**kw) for _ in range(S)]
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
            refs[5] = kn.Kde(**kw)
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
            if want is None:
                assert (fg[s] == 7).all(), (step, s)
                assert eng.frames_seen(s) == refs[s].fn  # frames since its (re)start
                continue
            assert np.array_equal(fg[s], want), (step, s, int((fg[s] != want).sum()))
            packed = np.packbits(want.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
            wbits = np.zeros(Wd * 8, np.uint8)
            wbits[:len(packed)] = packed
            assert np.array_equal(bits[s], wbits.view(np.uint64)), (step, s)
            assert eng.stream_flags(s) & capi.FG_VALID
    eng.close()


def test_two_1080p_streams_equal_restatement():
    torch = _torch()
    S, H, W, T = 2, 1080, 1920, 30
    clips = [scene(T, H, W, seed=70 + s) for s in range(S)]
    eng = Engine(capi.KDE, n_streams=S)
    eng.set_geometry(H, W, 3)
    def restate(clip):  # the two restatement runs side by side (numpy releases the GIL in its loops)
        k = kn.Kde()
        return [k.process(f) for f in clip]

    with ThreadPoolExecutor(S) as ex:
        wants = list(ex.map(restate, clips))
    Wd = H * W // 64
    for t in range(T):
        d = torch.from_numpy(np.stack([c[t] for c in clips])).cuda()
        d_fg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((S, Wd), dtype=torch.int64, device="cuda")
        flags = eng.process_batch_device(d, d_fg, None, d_bits)
        torch.cuda.synchronize()
        fg, bits = d_fg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            want = wants[s][t]
            assert (want is None) == (not flags & capi.FG_VALID), t
            if want is not None:
                assert np.array_equal(fg[s], want), (t, s, int((fg[s] != want).sum()))
                assert np.array_equal(bits[s], np.packbits(want.reshape(-1) != 0, bitorder="little").view(np.uint64)), (t, s)
    eng.close()


def test_demo_ustc_type_32_and_frame_processor_equal_fixture(tmp_path, golden_frames):
    """The host C++ layer: USTC_BGS(32) (tracker path) and FrameProcessor with enableKDE, against the reference's own masks."""
    import subprocess
    from test_gpu_01_host_cpp import HOST, DEMO, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    r, p, frames = golden_cases()["default"]
    want = masks_of(r)
    raw = str(tmp_path / "frames.raw")
    frames.tofile(raw)
    n, rows, cols = frames.shape[:3]
    ustc = tmp_path / "ustc"
    ustc.mkdir()
    res = subprocess.run([DEMO, raw, str(rows), str(cols), str(n), str(ustc / "out"), "32"], cwd=str(ustc), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.fromfile(str(ustc / "out.ustc.raw"), np.uint8).reshape(n, rows, cols)
    assert (got[:10] == 7).all() and np.array_equal(got[10:], want)  # learning frames: GetMask hands out no mask yet
    fp = tmp_path / "fp"
    write_fp_config(str(fp / "config"), set())
    with open(str(fp / "config" / "FrameProcessor.xml")) as f:
        xml = f.read().replace("</opencv_storage>", "<enableKDE>1</enableKDE>\n</opencv_storage>")
    with open(str(fp / "config" / "FrameProcessor.xml"), "w") as f:
        f.write(xml)
    res = subprocess.run([DEMO, raw, str(rows), str(cols), str(n), str(fp / "out")], cwd=str(fp), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.fromfile(str(fp / "out.KDE.raw"), np.uint8).reshape(n, rows, cols)
    assert (got[:10] == 7).all() and np.array_equal(got[10:], want)
    assert "<framesToLearn>10</framesToLearn>" in open(str(fp / "config" / "KDE.xml")).read()
