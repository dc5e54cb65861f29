"""T2FGMM_UM / T2FGMM_UV (BGS_T2FGMM_UM / BGS_T2FGMM_UV, USTC_BGS types 17 and 18) on the GPU against the outputs of the reference's
own tb/T2FGMM.cpp (tests/golden/t2f_ref.npz, read through tests/t2f_numpy.py; nothing here needs the reference tree) and against the
numpy restatement that tests/test_t2f_cpu.py holds to that fixture bit for bit.  Every comparison is exact: masks, mode counts and
the bits of every float of the modes below a pixel's count."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import t2f_numpy as tn
from gpu_helpers import _torch
from tracking_amd import Engine, capi

pytestmark = pytest.mark.gpu

ALGO = {"um": capi.T2FGMM_UM, "uv": capi.T2FGMM_UV}
ALL = [(typ, case) for typ in tn.TYPES for case in tn.cases()]
PKEYS = ("threshold", "alpha", "km", "kv", "gaussians")


def engine(typ, p, n_streams=1):
    e = Engine(ALGO[typ], n_streams=n_streams)
    e.set_t2f_params(**{k: p[k] for k in PKEYS})
    return e


@functools.lru_cache(maxsize=None)
def restated(typ, case, K=None):
    """(masks, modes [K*6][n], counts [n]) of the restatement on a fixture case's clip, optionally with another K: computed once."""
    r = tn.load()[typ, case]
    p = dict(r["params"], gaussians=K or r["params"]["gaussians"])
    masks, mdl = tn.run(typ, p, r["frames"])
    out = (masks, mdl.planes(), mdl.count.copy())
    for a in out:
        a.setflags(write=False)
    return out


def assert_model(eng, K, n, want_modes, want_count, where, stream=0):
    """Counts equal, and every float of the modes below a pixel's count equal bit for bit (the sixth, significants, included)."""
    cnt = eng.get_state("nmodes", (n,), np.uint8, stream=stream)
    assert np.array_equal(cnt, want_count), (where, "nmodes", int((cnt != want_count).sum()))
    got = eng.get_state("modes", (K * tn.FIELDS, n), np.float32, stream=stream)
    below = tn.below_count(None, cnt, K).reshape(K * tn.FIELDS, n)
    a, b = got.view(np.uint32)[below], np.asarray(want_modes).view(np.uint32)[below]
    assert np.array_equal(a, b), (where, "modes: %d of %d floats below the count differ" % (int((a != b).sum()), a.size))


def words_of(mask, Wd):
    packed = np.packbits(mask.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
    w = np.zeros(Wd * 8, np.uint8)
    w[:len(packed)] = packed
    return w.view(np.uint64)


@pytest.mark.parametrize("typ,case", ALL, ids=["%s-%s" % tc for tc in ALL])
def test_host_path_matches_reference_fixture(typ, case):
    r = tn.load()[typ, case]
    frames, p = r["frames"], r["params"]
    n = frames.shape[1] * frames.shape[2]
    eng = engine(typ, p)
    for t, f in enumerate(frames):
        fg, bg = eng.process(f, want_bg=False)
        assert bg is None and np.array_equal(fg, r["masks"][t]), "frame %d: %d mask pixels differ" % (t, int((fg != r["masks"][t]).sum()))
    if "modes" in r:
        assert_model(eng, p["gaussians"], n, r["modes"], r["nmodes"], (typ, case, "fixture"))
    _, modes, count = restated(typ, case)  # the cases too large for stored planes have only this
    assert_model(eng, p["gaussians"], n, modes, count, (typ, case, "restatement"))
    eng.close()


@pytest.mark.parametrize("typ", tn.TYPES)
def test_batch_path_streams_of_different_ages_share_state_tiles(typ):
    """S = 3 streams of 37 x 53 = 1 961 pixels: pixels of two streams lie in tiles 7 and 15 and the launch covers 5 883 pixels (no
    multiple of 64 or 256).  Stream k enters the clip k frames late (ragged, ragged_o1, ragged_o2); stream 1 is reset before frame 6,
    so its model is rebuilt from that frame on while the others go on: from there it is compared with a fresh restatement."""
    torch = _torch()
    cases = tn.load()
    rs = [cases[typ, c] for c in ("ragged", "ragged_o1", "ragged_o2")]
    S, (T, H, W) = 3, rs[0]["masks"].shape
    n, words = H * W, (H * W + 63) // 64
    assert n % 256 and (n - 1) // 256 == n // 256
    p = rs[0]["params"]
    eng = engine(typ, p, n_streams=S)
    eng.set_geometry(H, W, 3)
    reset_at, fresh = 6, tn.model_of(typ, p, n)
    for t in range(T):
        if t == reset_at:
            eng.reset_stream(1)
        d_frames = torch.from_numpy(np.stack([r["frames"][t] for r in rs])).cuda()
        d_fg = torch.full((S, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((S, words), -1, dtype=torch.int64, device="cuda")
        flags = eng.process_batch_device(d_frames, d_fg, None, d_bits)
        torch.cuda.synchronize()
        assert flags == capi.FG_VALID
        fg = d_fg.cpu().numpy()
        bits = d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            want = rs[s]["masks"][t]
            if s == 1 and t >= reset_at:
                want = fresh.step(rs[1]["frames"][t]).reshape(H, W)
            assert np.array_equal(fg[s], want), (t, s, int((fg[s] != want).sum()))
            assert np.array_equal(bits[s], words_of(want, words)), (t, s)
    assert [eng.frames_seen(s) for s in range(S)] == [T, T - reset_at, T]
    for s, case in ((0, "ragged"), (2, "ragged_o2")):
        _, modes, count = restated(typ, case)
        assert_model(eng, p["gaussians"], n, modes, count, (typ, "stream", s), stream=s)
    assert_model(eng, p["gaussians"], n, fresh.planes(), fresh.count, (typ, "stream 1 after its reset"), stream=1)
    eng.close()


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("case", ["tile", "ragged"])
@pytest.mark.parametrize("typ", tn.TYPES)
def test_clip_of_15_frames_equals_the_frame_by_frame_run(typ, case, K):
    """15 frames = 8 + 4 + 2 + 1: three fused launches that keep the model in registers and one per-frame launch; with
    BGS_OPT_CLIP_FUSE 0 fifteen per-frame launches.  Masks of every frame, packed words and the final model equal the frame-by-frame
    run (one process_batch_device call per frame) and the restatement, for every K the kernel is built for."""
    torch = _torch()
    r = tn.load()[typ, case]
    frames, p = r["frames"][:15], dict(r["params"], gaussians=K)
    T, H, W = frames.shape[:3]
    n, Wd = H * W, (H * W + 63) // 64
    want_masks, want_modes, want_count = restated(typ, case, K)
    assert T == 15 and len(want_masks) == 15
    d_all = torch.from_numpy(np.array(frames)).cuda().unsqueeze(1)  # [T][1][H][W][3]
    step = engine(typ, p)
    step.set_geometry(H, W, 3)
    for t in range(T):
        d_fg = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        assert step.process_batch_device(d_all[t], d_fg, None, None) == capi.FG_VALID
        torch.cuda.synchronize()
        assert np.array_equal(d_fg.cpu().numpy()[0], want_masks[t]), (t, "frame by frame")
    assert_model(step, K, n, want_modes, want_count, (typ, case, K, "frame by frame"))
    step_modes = step.get_state("modes", (K * tn.FIELDS, n), np.float32)
    step.close()
    for fuse, launches in ((1, 4), (0, 15)):
        eng = engine(typ, p)
        eng.set_geometry(H, W, 3)
        eng.set_option(capi.OPT_CLIP_FUSE, fuse)
        eng.enable_kernel_timing(True)
        d_fg = torch.full((T, 1, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((T, 1, Wd), -1, dtype=torch.int64, device="cuda")
        flags = eng.process_clip_device(d_all, T, d_fg, None, d_bits)
        torch.cuda.synchronize()
        assert flags == [capi.FG_VALID] * T and eng.frames_seen(0) == T
        _, nl, name = eng.kernel_timing()
        assert nl == launches and name == "t2f_gmm_kernel", (fuse, nl, name)  # the last launch is the single left-over frame
        fg, bits = d_fg.cpu().numpy()[:, 0], d_bits.cpu().numpy().view(np.uint64)[:, 0]
        for t in range(T):
            assert np.array_equal(fg[t], want_masks[t]), (fuse, t, int((fg[t] != want_masks[t]).sum()))
            assert np.array_equal(bits[t], words_of(want_masks[t], Wd)), (fuse, t)
        assert_model(eng, K, n, want_modes, want_count, (typ, case, K, "fuse %d" % fuse))
        assert eng.get_state("modes", (K * tn.FIELDS, n), np.float32).tobytes() == step_modes.tobytes()  # above the count too
        eng.close()


@pytest.mark.parametrize("typ", tn.TYPES)
def test_a_fused_run_is_one_launch_named_as_a_clip(typ):
    """14 frames = 8 + 4 + 2: three launches, all of the clip form."""
    torch = _torch()
    r = tn.load()[typ, "tile"]
    T, H, W = 14, 16, 64
    eng = engine(typ, r["params"])
    eng.set_geometry(H, W, 3)
    eng.enable_kernel_timing(True)
    d_fg = torch.zeros((T, 1, H, W), dtype=torch.uint8, device="cuda")
    eng.process_clip_device(torch.from_numpy(np.array(r["frames"][:T])).cuda().unsqueeze(1), T, d_fg, None, None)
    torch.cuda.synchronize()
    _, nl, name = eng.kernel_timing()
    assert nl == 3 and "clip" in name, (nl, name)
    assert np.array_equal(d_fg.cpu().numpy()[:, 0], r["masks"][:T])
    eng.close()


@pytest.mark.parametrize("case", ["tile", "tiny5x7"])
@pytest.mark.parametrize("typ", tn.TYPES)
def test_packed_words_equal_the_packed_byte_mask(typ, case):
    """16 x 64: the kernel writes the words; 5 x 7: the engine packs them from bytes.  With and without a byte mask asked for."""
    torch = _torch()
    r = tn.load()[typ, case]
    T, H, W = r["masks"].shape
    Wd = (H * W + 63) // 64
    both, packed = engine(typ, r["params"]), engine(typ, r["params"])
    for e in (both, packed):
        e.set_geometry(H, W, 3)
    for t in range(T):
        d_frame = torch.from_numpy(np.array(r["frames"][t][None])).cuda()
        d_fg = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        b1 = torch.full((1, Wd), -1, dtype=torch.int64, device="cuda")
        b2 = torch.full((1, Wd), -1, dtype=torch.int64, device="cuda")
        assert both.process_batch_device(d_frame, d_fg, None, b1) == capi.FG_VALID
        assert packed.process_batch_device(d_frame, None, None, b2) == capi.FG_VALID
        torch.cuda.synchronize()
        assert np.array_equal(d_fg.cpu().numpy()[0], r["masks"][t]), t
        want = words_of(r["masks"][t], Wd)
        assert np.array_equal(b1.cpu().numpy().view(np.uint64)[0], want) and np.array_equal(b2.cpu().numpy().view(np.uint64)[0], want), t
    both.close(), packed.close()


def test_gray_frames_and_groups_are_refused_with_the_class_name():
    for typ, name in tn.CLASS_NAMES.items():
        eng = Engine(ALGO[typ])
        with pytest.raises(capi.BgsError) as ei:
            eng.process(np.zeros((12, 16), np.uint8))
        assert ei.value.code == capi.ERR_UNSUPPORTED and name in str(ei.value)
        fg, bg = eng.process(np.zeros((4, 4, 3), np.uint8))  # still usable
        assert bg is None and (fg == 255).all()  # the first frame has no mode to match: all foreground
        eng.close()
        algos = (C.c_int * 2)(capi.FRAME_DIFF, ALGO[typ])
        g = C.c_void_p()
        assert capi.lib().bgs_group_create(algos, None, 2, 0, 1, C.byref(g)) == capi.ERR_UNSUPPORTED
        assert name.encode() in capi.lib().bgs_last_error()
    with pytest.raises(capi.BgsError):
        Engine(capi.VUMETER).set_t2f_params(gaussians=2)


@pytest.mark.parametrize("typ", tn.TYPES)
def test_parameters_set_after_the_first_frame_leave_the_frozen_values_in_force(typ):
    """The wrappers hand their members to the model inside `if(firstTime)` only: other values at frame 5 are accepted and change
    nothing - masks and model still equal the reference's for the first values, and get returns those."""
    r = tn.load()[typ, "tile"]
    frames, p = r["frames"], r["params"]
    eng = engine(typ, p)
    for t, f in enumerate(frames):
        if t == 5:
            eng.set_t2f_params(threshold=2.0, alpha=0.4, km=3.0, kv=0.3, gaussians=5)
            with pytest.raises(capi.BgsError):  # a refusal stays a refusal
                eng.set_t2f_params(gaussians=6)
        fg, _ = eng.process(f, want_bg=False)
        assert np.array_equal(fg, r["masks"][t]), t
    q = eng.get_t2f_params()
    assert (q.threshold, q.alpha, q.km, q.kv, q.gaussians) == (p["threshold"], p["alpha"], np.float32(p["km"]), np.float32(p["kv"]), p["gaussians"])
    assert_model(eng, p["gaussians"], frames.shape[1] * frames.shape[2], r["modes"], r["nmodes"], (typ, "frozen"))
    eng.close()


@pytest.mark.parametrize("typ,ustc", [("um", 17), ("uv", 18)])
def test_host_classes_equal_the_fixture_and_round_trip_their_xml(tmp_path, typ, ustc):
    """The C++ host layer: USTC_BGS(17 / 18) (the tracker's path) with the defaults on frames_96x80 - the XML it writes holds the
    reference's keys in the reference's order - and FrameProcessor with enableT2FGMM_U*, the thr2_km3_kv03 case's values through
    ./config/T2FGMM_U*.xml, which must come back unchanged."""
    from test_gpu_01_host_cpp import DEMO, HOST, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    name = tn.CLASS_NAMES[typ]
    keys = ["threshold", "alpha", "km", "kv", "gaussians", "showOutput"]
    for mode, case in (("ustc", "default"), ("fp", "thr2_km3_kv03")):
        r = tn.load()[typ, case]
        n, rows, cols = r["masks"].shape
        wd = tmp_path / mode
        (wd / "config").mkdir(parents=True)
        raw = str(wd / "frames.raw")
        r["frames"].tofile(raw)
        if mode == "ustc":
            args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out"), str(ustc)]
            out = wd / "out.ustc.raw"
        else:
            p = r["params"]
            (wd / "config" / (name + ".xml")).write_text(
                '<?xml version="1.0"?>\n<opencv_storage>\n<threshold>%r</threshold>\n<alpha>%r</alpha>\n<km>%r</km>\n<kv>%r</kv>\n<gaussians>%d</gaussians>\n<showOutput>0</showOutput>\n</opencv_storage>\n'
                % (p["threshold"], p["alpha"], p["km"], p["kv"], p["gaussians"]))
            write_fp_config(str(wd / "config"), set())
            path = str(wd / "config" / "FrameProcessor.xml")
            text = open(path).read().replace("</opencv_storage>", "<enable%s>1</enable%s>\n</opencv_storage>" % (name, name))
            open(path, "w").write(text)
            args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out")]
            out = wd / ("out.%s.raw" % name)
        res = subprocess.run(args, cwd=str(wd), capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        assert name + "()" in res.stdout and "~" + name + "()" in res.stdout  # the reference's banners
        got = np.fromfile(str(out), np.uint8).reshape(n, rows, cols)
        assert np.array_equal(got, r["masks"]), (mode, int((got != r["masks"]).sum()))
        saved = (wd / "config" / (name + ".xml")).read_text()
        pos = [saved.index("<%s>" % k) for k in keys]
        assert pos == sorted(pos), saved
        if mode == "ustc":
            for frag in ("<threshold>9.</threshold>", "<alpha>", "<km>1.5</km>", "<gaussians>3</gaussians>", "<showOutput>1</showOutput>"):
                assert frag in saved, saved
        else:
            assert "<threshold>2.</threshold>" in saved and "<km>3.</km>" in saved and "<showOutput>0</showOutput>" in saved, saved
