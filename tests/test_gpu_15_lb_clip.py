"""bgs_process_clip_device on the five package_bgs/lb/ classes (BGS_LB_*, USTC_BGS types 25-29): runs of 8 / 4 / 2 frames go
through one lb_*_clip_kernel launch that keeps the pixel's model in registers (kernel_lb.h), what is left over takes the per-frame
kernel.  The models are strictly per pixel, so a fused run computes what the frame-by-frame launches compute: bit for bit against
BGS_OPT_CLIP_FUSE 0 (both run the same device exp()), and against the reference's fixtures and the numpy restatement under the
contract of test_gpu_11_lb.py (exact, the fuzzy classes' model planes within lb_numpy.FUZZY_PLANE_TOL)."""
import numpy as np
import pytest

import lb_numpy as ln
from test_gpu_11_lb import assert_planes, engine, params_of, planes_of
from test_lb_cpu import CASES, CLASSES, WHOLE_MODEL, golden, masks_of
from tracking_amd import capi

from gpu_helpers import _torch

pytestmark = pytest.mark.gpu

BOTH = capi.FG_VALID | capi.BG_VALID
PER_FRAME = {25: "lb_gauss_kernel", 26: "lb_fuzzy_gauss_kernel", 27: "lb_mog_kernel", 28: "lb_som_kernel", 29: "lb_fuzzy_som_kernel"}


def slab_of(clips, t0, n):
    """clips [S][T][H][W][3] -> device slab [n][S][H][W][3] of frames t0 .. t0 + n"""
    return _torch().from_numpy(np.ascontiguousarray(np.stack([c[t0:t0 + n] for c in clips], 1))).cuda()


def run_clip(eng, d_frames, n, S, H, W, first=0, count=None, bits=True):
    """One clip call with every output -> (masks [n][S][H][W], backgrounds, packed words [n][S][Wd] or None, flags)"""
    torch = _torch()
    Wd = (H * W + 63) // 64
    d_fg = torch.full((n, S, H, W), 7, dtype=torch.uint8, device="cuda")
    d_bg = torch.full((n, S, H, W, 3), 9, dtype=torch.uint8, device="cuda")
    d_bits = torch.zeros((n, S, Wd), dtype=torch.int64, device="cuda") if bits else None
    flags = eng.process_clip_device(d_frames, n, d_fg, d_bg, d_bits, first=first, count=count)
    torch.cuda.synchronize()
    return d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64) if bits else None, flags


def words_of(mask, Wd):
    packed = np.packbits(mask.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
    w = np.zeros(Wd * 8, np.uint8)
    w[:len(packed)] = packed
    return w.view(np.uint64)


@pytest.mark.parametrize("cls", CLASSES)
def test_clip_runs_of_8_4_2_frames_are_one_launch_each(cls):
    """14 frames = 8 + 4 + 2: three launches of the clip kernel; with BGS_OPT_CLIP_FUSE 0 fourteen of the per-frame kernel; a
    15-frame clip ends with one per-frame launch."""
    S, H, W = 2, 16, 64
    clips = [ln.noisy_clip(15, H, W, seed=1500 + 10 * cls + s) for s in range(S)]
    seen = {}
    for fuse, T in ((None, 14), (0, 14), (None, 15)):
        eng = engine(cls, n_streams=S)
        eng.set_geometry(H, W, 3)
        if fuse is not None:
            eng.set_option(capi.OPT_CLIP_FUSE, fuse)
        eng.enable_kernel_timing(True)
        fg, bg, bits, flags = run_clip(eng, slab_of(clips, 0, T), T, S, H, W)
        assert flags == [BOTH] * T
        seen[(fuse, T)] = eng.kernel_timing()[1:] + (fg, bg, bits)
        assert [eng.frames_seen(s) for s in range(S)] == [T, T]
        eng.close()
    n, name = seen[(None, 14)][:2]
    assert n == 3 and "clip" in name, (n, name)
    assert seen[(0, 14)][:2] == (14, PER_FRAME[cls])
    assert seen[(None, 15)][:2] == (4, PER_FRAME[cls])
    for a, b in zip(seen[(None, 14)][2:], seen[(0, 14)][2:]):
        assert np.array_equal(a, b)


# BGS_LB_PX (pixels per lane) concerns the two Gaussian kernels only: both forms for them
@pytest.mark.parametrize("geom", [(24, 64), (10, 13), (37, 53)])
@pytest.mark.parametrize("cls,px", [(c, px) for c in CLASSES for px in ((2, 1) if c in (25, 26) else (1,))])
def test_fused_equals_unfused_bit_for_bit(cls, px, geom, monkeypatch):
    """23 frames (8 + 8 + 4 + 2 + 1) of streams 1..3 out of 5, so the slab stride differs from the run's size.  24 x 64: words from
    the kernel; 10 x 13: even n, ragged words; 37 x 53: odd n (one pixel per lane whatever BGS_LB_PX says), a partial last
    workgroup.  The SOMs' schedule crosses into the online phase inside the first fused launch."""
    monkeypatch.setenv("BGS_LB_PX", str(px))
    H, W = geom
    S, T, n = 5, 23, H * W
    kw = dict(training_steps=6) if cls in (28, 29) else {}
    clips = [ln.noisy_clip(T, H, W, seed=1600 + 10 * cls + s, box=0.15) for s in range(S)]
    d_frames = slab_of(clips[1:4], 0, T)
    res = []
    for fuse in (1, 0):
        eng = engine(cls, n_streams=S, **kw)
        eng.set_geometry(H, W, 3)
        eng.set_option(capi.OPT_CLIP_FUSE, fuse)
        fg, bg, bits, flags = run_clip(eng, d_frames, T, 3, H, W, first=1, count=3)
        assert flags == [BOTH] * T
        assert [eng.frames_seen(s) for s in range(S)] == [0, T, T, T, 0]
        res.append((fg, bg, bits, [planes_of(eng, cls, n, s) for s in (1, 2, 3)]))
        eng.close()
    (fg, bg, bits, planes), (ufg, ubg, ubits, uplanes) = res
    assert set(np.unique(ufg)) == {0, 255}
    assert np.array_equal(fg, ufg) and np.array_equal(bg, ubg) and np.array_equal(bits, ubits)
    for t in range(T):
        for s in range(3):
            assert np.array_equal(bits[t, s], words_of(fg[t, s], bits.shape[2])), (t, s)
    for a, b in zip(planes, uplanes):
        assert set(a) == set(b)
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), (cls, geom, name)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cls", CLASSES)
def test_clip_calls_equal_reference_fixture(cls, case):
    """test_engine_equals_reference_fixture's contract with clip calls of 11 frames (8 + 2 + 1) in place of process(); the `change`
    case starts a new call at the frame where its parameters switch."""
    r, p, change, frames = golden(cls, case)
    T, H, W = frames.shape[:3]
    eng = engine(cls, **p)
    eng.set_geometry(H, W, 3)
    want = masks_of(r)
    d_all = _torch().from_numpy(np.ascontiguousarray(frames)).cuda().unsqueeze(1)  # [T][1][H][W][3]
    t = 0
    while t < T:
        if change and t == change[0]:
            eng.set_params(params_of(cls, **dict(p, **change[1])))
        n = min(11, T - t)
        if change and t < change[0]:
            n = min(n, change[0] - t)
        fg, bg, _, flags = run_clip(eng, d_all[t:t + n], n, 1, H, W, bits=False)
        assert flags == [BOTH] * n
        for j in range(n):
            assert np.array_equal(fg[j, 0], want[t + j]), (cls, case, t + j, int((fg[j, 0] != want[t + j]).sum()))
            assert ln.crc(bg[j, 0]) == int(r["bg_crc32"][t + j]), (cls, case, t + j)
        t += n
    assert np.array_equal(bg[-1, 0], r["bg_last"])
    if case in WHOLE_MODEL:
        want_planes = {k: r[k] for k in planes_of(eng, cls, H * W) if k in r}
        assert len(want_planes) >= 2
        assert_planes(cls, planes_of(eng, cls, H * W), want_planes, (cls, case))
    eng.close()


@pytest.mark.parametrize("cls", CLASSES)
def test_init_inside_a_run_reset_ages_and_single_frames(cls):
    """9 frames from seen == 0 (Init inside the fused launch of 8), reset_stream(2), 12 frames with stream 2 younger than the
    others (three runs of one age), single frames, one more clip: after every call every mask, background, packed word, plane
    and the SOMs' counter equal one restatement per stream."""
    torch = _torch()
    S, H, W = 4, 37, 53
    n, Wd = H * W, (H * W + 63) // 64
    kw = dict(training_steps=6) if cls in (28, 29) else {}
    clips = [ln.noisy_clip(32, H, W, seed=1700 + 10 * cls + s, box=0.15) for s in range(S)]
    eng = engine(cls, n_streams=S, **kw)
    eng.set_geometry(H, W, 3)
    refs = [ln.LB(cls, **kw) for _ in range(S)]
    t0 = 0

    def check_state(where):
        for s in range(S):
            assert eng.frames_seen(s) == refs[s].fn and eng.stream_flags(s) == BOTH, (where, s)
            assert_planes(cls, planes_of(eng, cls, n, s), refs[s].planes(), (cls, where, s))

    def clip(nf, where):
        fg, bg, bits, flags = run_clip(eng, slab_of(clips, t0, nf), nf, S, H, W)
        assert flags == [BOTH] * nf
        for j in range(nf):
            for s in range(S):
                wfg, wbg = refs[s].process(clips[s][t0 + j])
                assert np.array_equal(fg[j, s], wfg), (cls, where, j, s, int((fg[j, s] != wfg).sum()))
                assert np.array_equal(bg[j, s], wbg), (cls, where, j, s)
                assert np.array_equal(bits[j, s], words_of(wfg, Wd)), (cls, where, j, s)
        check_state(where)
        return t0 + nf

    t0 = clip(9, "first")
    eng.reset_stream(2)
    refs[2] = ln.LB(cls, **kw)
    t0 = clip(12, "after reset")
    for _ in range(3):
        d_fg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
        d_bg = torch.zeros((S, H, W, 3), dtype=torch.uint8, device="cuda")
        eng.process_batch_device(torch.from_numpy(np.stack([c[t0] for c in clips])).cuda(), d_fg, d_bg, None)
        torch.cuda.synchronize()
        for s in range(S):
            wfg, wbg = refs[s].process(clips[s][t0])
            assert np.array_equal(d_fg.cpu().numpy()[s], wfg) and np.array_equal(d_bg.cpu().numpy()[s], wbg), (cls, t0, s)
        t0 += 1
    check_state("single frames")
    clip(6, "last")
    eng.close()


def test_mog_write_set_is_the_union_over_the_run():
    """Pixels that dwell on four colours: K grows to 3, the last slot is replaced, swaps happen - inside two fused launches of 8.
    A slot that one frame of the run changed and the last one did not must still be written."""
    H, W, T = 13, 11, 16
    kw = dict(learning_rate=180, noise_variance=40)
    frames = ln.modes_clip(T, H, W, seed=1800)
    eng, ref = engine(27, **kw), ln.LB(27, **kw)
    eng.set_geometry(H, W, 3)
    eng.enable_kernel_timing(True)
    fg, bg, _, _ = run_clip(eng, slab_of([frames], 0, T), T, 1, H, W)
    assert eng.kernel_timing()[1:] == (2, "lb_mog_clip_kernel")
    for t in range(T):
        wfg, wbg = ref.process(frames[t])
        assert np.array_equal(fg[t, 0], wfg) and np.array_equal(bg[t, 0], wbg), t
    assert ref.swaps > 0 and ref.replaced > 0 and int(ref.k.max()) == 3
    got, want = planes_of(eng, 27, H * W), ref.planes()
    for name in ("w", "mu", "var", "sortkey", "k"):
        assert np.array_equal(got[name], np.asarray(want[name]).reshape(got[name].shape)), name
    eng.close()


@pytest.mark.parametrize("cls", [28, 29])
def test_som_streams_of_one_age_with_different_training_counters_take_the_per_frame_launches(cls):
    """trainingSteps changed between calls that fed the two streams separately: both have seen 5 frames, m_K is 3 and 5.  The
    8-frame run cannot share one schedule, so it runs as 8 per-frame launches with the per-stream table - same results."""
    torch = _torch()
    S, H, W = 2, 16, 24
    clips = [ln.noisy_clip(13, H, W, seed=1900 + 10 * cls + s, box=0.15) for s in range(S)]
    eng = engine(cls, n_streams=S, training_steps=2)
    eng.set_geometry(H, W, 3)
    refs = [ln.LB(cls, training_steps=2) for _ in range(S)]
    for s in range(S):
        if s == 1:
            eng.set_params(params_of(cls, training_steps=10))
            for r in refs:
                r.set(training_steps=10)
        for t in range(5):
            eng.process_batch_device(torch.from_numpy(clips[s][t]).cuda().unsqueeze(0), None, None, None, first=s, count=1)
            refs[s].process(clips[s][t])
    assert [int(planes_of(eng, cls, H * W, s)["count"][0]) for s in range(S)] == [3, 5]
    eng.enable_kernel_timing(True)
    fg, bg, bits, flags = run_clip(eng, slab_of([c[5:] for c in clips], 0, 8), 8, S, H, W)
    assert flags == [BOTH] * 8 and eng.kernel_timing()[1:] == (8, PER_FRAME[cls])
    for t in range(8):
        for s in range(S):
            wfg, wbg = refs[s].process(clips[s][5 + t])
            assert np.array_equal(fg[t, s], wfg) and np.array_equal(bg[t, s], wbg), (cls, t, s)
            assert np.array_equal(bits[t, s], words_of(wfg, H * W // 64)), (cls, t, s)
    for s in range(S):
        assert_planes(cls, planes_of(eng, cls, H * W, s), refs[s].planes(), (cls, "end", s))
    eng.close()
