"""MOG2 filter kernel, multi-record path (kernel_mog2.h, mog2_stream): a wave in which some lane needs more than one record no longer
holds five records per lane; it streams the slots 0 .. 4 through two registers' worth of float4, keeps the comparisons as bit masks,
reads the matched record again from its slot, and takes the summaries of a pixel whose summaries were not valid from the records as
they land.  No wave of the benchmark input takes that path, so these tests drive it at the smallest shapes that reach it.

Everything is compared with the CPU oracle: masks bit for bit on every frame, the model state within 1e-4 at the end
(gpu_helpers.check_mog2_state), at sparse level 4 the summaries' invariants over the whole frame.  Each test also shows ON THE CPU,
from the oracle's state and the frame alone, that its input reaches the path it is for: `_survivors` restates the rejection rule in
numpy (buckets >> 3, S = sum of the absolute bucket differences over the three channels, a live mode is ruled out iff its variance is
<= 24 - class 0 when a summary is taken - and S >= s_min).  s_min comes from the kernel header's own mog2_smin(mog2_tq(.)), through a
stand-alone host program as in test_mog2_smin_cpu.py."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import pyoracle
from tracking_amd import Engine, capi

from gpu_helpers import *  # noqa: F401,F403
from gpu_helpers import _params, _torch
from test_gpu_00_configs import _mog2_summary_invariants
from test_gpu_18_mog2_lean import _sat_like

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@functools.lru_cache(maxsize=None)
def _s_min(tmax):
    """mog2_smin(mog2_tq(tmax)) as the host computes it for a launch (engine_mog2.h, mog2_fill_args)."""
    prog = '#include "kernel_mog2.h"\n#include <cstdio>\nint main() { std::printf("%%u\\n", bgs::mog2_smin(bgs::mog2_tq(%rf))); return 0; }\n' % float(tmax)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "smin.hip"), os.path.join(d, "smin")
        with open(src, "w") as f:
            f.write(prog)
        cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "tracking_amd", "csrc"), "-o", exe, src]
        build = subprocess.run(cmd, capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-2000:]
        run = subprocess.run([exe], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        return int(run.stdout.strip())


def _default_s_min():
    p = capi.default_params(capi.MOG2)
    return _s_min(max(p.mog2_var_threshold, p.mog2_var_threshold_gen))


def _survivors(orc, frame, n, s_min, empty=False):
    """Per pixel: the records the summaries leave for `frame`, from the oracle's model BEFORE it processes that frame (`empty`: before
    its first frame, when there is no model yet)."""
    if empty:
        return np.zeros(n, np.int64), np.zeros(n, np.int32)
    nm = orc.get_state("nmodes", (n,), np.uint8).astype(np.int32)
    mu = orc.get_state("mu", (5, 3, n), np.float32)
    var = orc.get_state("var", (5, n), np.float32)
    live = np.arange(5)[:, None] < nm[None, :]
    inside = np.all((mu >= 0) & (mu < 256), axis=1)
    q = np.where(inside[:, None, :], np.floor(np.where(live[:, None, :], mu, 0)).astype(np.int64) >> 3, 0)
    xq = frame.reshape(n, 3).T.astype(np.int64) >> 3
    S = np.abs(q - xq[None]).sum(axis=1)
    out = inside & (var <= 24.0) & (S >= s_min)
    return (live & ~out).sum(axis=0), nm


# spacing of a pixel's levels: it changes every 8 columns over 6, 10, 14, 20, 28 and 40 levels.  The bands run on from one row into the
# next (80 columns = 10 bands, the pattern has 16): 64 model pixels in which neighbouring lanes need five, two or one record are followed
# by 64 whose modes lie 28 and 40 apart - one record each, the one-record form - so both forms of the kernel run in every launch.
_BANDS = np.array([6, 10, 14, 20, 28, 40, 6, 10, 28, 40, 28, 40, 28, 40, 28, 40])


def _banded(T, H, W, seed, spacing=None):
    """Per pixel up to five levels `spacing` apart, its own phase, noise +-2; 3, then 4, then 5 levels in play (ten frames each); in
    every frame 2 % of the pixels show a value at least 60 levels from every level of theirs (no record survives: a mode is created)."""
    rng = np.random.default_rng(seed)
    n = H * W
    if spacing is None:
        spacing = _BANDS[(np.arange(n) // 8) % len(_BANDS)]
    spacing = np.broadcast_to(np.asarray(spacing), (n,)).reshape(H, W, 1)
    base = rng.integers(10, 20, (H, W, 1))
    phase = rng.integers(0, 5, (H, W, 1))
    frames = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        lvl = (t + phase) % min(5, 3 + t // 10)
        f = base + spacing * lvl + rng.integers(-2, 3, (H, W, 3))
        far = rng.random((H, W, 1)) < 0.02
        f = np.where(far, base + 4 * spacing + 64 + rng.integers(0, 6, (H, W, 1)), f)  # at most 19 + 160 + 69
        assert f.min() >= 0 and f.max() <= 255
        frames[t] = f.astype(np.uint8)
    return frames


def _path_counts(surv_by_frame, first_frame=15):
    """Over the frames from `first_frame` on, per 64-pixel group of model pixels: groups with a pixel of two or more surviving records,
    groups with none, pixel-frames with zero surviving records, the largest number of surviving records."""
    multi = none = zero = most = groups = 0
    for t, surv in enumerate(surv_by_frame):
        if t < first_frame:
            continue
        g = surv.reshape(-1, 64)
        has = (g >= 2).any(axis=1)
        multi += int(has.sum())
        none += int((~has).sum())
        groups += g.shape[0]
        zero += int((surv == 0).sum())
        most = max(most, int(surv.max()))
    return multi, none, groups, zero, most


def _run_banded(levels, T=30, H=16, W=80, seed=3, after_launch=None):
    """The banded input through one engine, sparse level levels[t % len(levels)] at frame t, against the oracle.  Returns the surviving
    records per pixel and frame (CPU side)."""
    torch = _torch()
    n = H * W
    assert n % 64 == 0
    frames = _banded(T, H, W, seed)
    s_min = _default_s_min()
    eng = Engine(capi.MOG2)
    eng.set_geometry(H, W, 3)
    orc = pyoracle.Oracle(capi.MOG2)
    d_fg = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    surv_by_frame = []
    for t in range(T):
        level = levels[t % len(levels)]
        eng.set_option(capi.OPT_MOG2_SPARSE, level)
        surv, nm = _survivors(orc, frames[t], n, s_min, empty=t == 0)
        surv_by_frame.append(surv)
        assert eng.process_batch_device(torch.from_numpy(frames[t:t + 1]).cuda(), d_fg, None, None) & capi.FG_VALID
        torch.cuda.synchronize()
        ofg, _ = orc.process(frames[t], want_bg=False)
        got = d_fg[0].cpu().numpy()
        assert np.array_equal(got, ofg), (level, t, int((got != ofg).sum()))
        if after_launch is not None:
            after_launch(eng, t, level, levels[(t - 1) % len(levels)] if t else None, nm)
    check_mog2_state(eng, orc, n)
    return eng, surv_by_frame


def _assert_mixed(surv_by_frame):
    multi, none, groups, zero, most = _path_counts(surv_by_frame)
    assert 4 * multi >= groups, (multi, groups)
    assert none >= 1
    assert zero >= 20, zero
    assert most == 5, most


def test_mixed_waves_one_tile_and_a_few_more():
    """16 x 80 pixels = five tiles, twenty waves, level 4.  Waves whose lanes need five, two, one and no record beside waves that take
    the one-record form; pixels without a surviving record create a mode."""
    n = 16 * 80
    eng, surv = _run_banded([4])
    _assert_mixed(surv)
    assert _mog2_summary_invariants(eng, n) == 1.0
    eng.close()


def test_rebuild_while_streaming():
    """The sparse level alternates 2, 2, 4, 4, 1, 4 from launch to launch: every level-4 launch that follows another level finds every
    valid bit clear, loads every live record and rebuilds all summaries from the records as they stream by; the level-4 launch after
    it filters with them."""
    n = 16 * 80
    rebuilt = []

    def after_launch(eng, t, level, before, nm):
        vfrac = _mog2_summary_invariants(eng, n)
        if level == 4:
            assert vfrac == 1.0, (t, vfrac)  # summary_valid is 1 for every pixel, and every summary covers its record
            if before is not None and before != 4 and t >= 15:
                # the launch rebuilt: on entry no pixel's summaries were valid, and some 64-pixel group held a pixel with several modes
                rebuilt.append(int((nm.reshape(-1, 64) >= 2).any(axis=1).sum()))
        else:
            assert vfrac == 0.0, (t, level, vfrac)

    eng, surv = _run_banded([2, 2, 4, 4, 1, 4], after_launch=after_launch)
    _assert_mixed(surv)
    assert len(rebuilt) >= 4 and min(rebuilt) >= 1, rebuilt
    assert _mog2_summary_invariants(eng, n) == 1.0  # frame 29 is a level-4 launch
    eng.close()


def test_filter_kernel_equals_the_eager_kernel_bitwise():
    """Exactness against the project's own other path: an engine at level 4 and one at level 1 run the same 40 frames; weights,
    variances, means, mode counts and masks are equal bit for bit."""
    torch = _torch()
    H, W, T = 16, 80, 40
    n = H * W
    frames = _banded(T, H, W, seed=3)
    s_min = _default_s_min()
    orc = pyoracle.Oracle(capi.MOG2)
    engs = []
    for level in (4, 1):
        e = Engine(capi.MOG2)
        e.set_geometry(H, W, 3)
        e.set_option(capi.OPT_MOG2_SPARSE, level)
        engs.append((e, torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")))
    surv_by_frame = []
    for t in range(T):
        surv_by_frame.append(_survivors(orc, frames[t], n, s_min, empty=t == 0)[0])
        orc.process(frames[t], want_bg=False)
        d = torch.from_numpy(frames[t:t + 1]).cuda()
        for e, fg in engs:
            assert e.process_batch_device(d, fg, None, None) & capi.FG_VALID
        torch.cuda.synchronize()
        assert np.array_equal(engs[0][1].cpu().numpy(), engs[1][1].cpu().numpy()), t
        if t + 1 in (10, 25, 40):
            for plane, shape, dt in (("w", (5, n), np.float32), ("var", (5, n), np.float32), ("mu", (5, 3, n), np.float32), ("nmodes", (n,), np.uint8)):
                a, b = engs[0][0].get_state(plane, shape, dt), engs[1][0].get_state(plane, shape, dt)
                assert np.array_equal(a.view(np.uint32 if dt == np.float32 else np.uint8), b.view(np.uint32 if dt == np.float32 else np.uint8)), (plane, t + 1)
    _assert_mixed(surv_by_frame)
    for e, _ in engs:
        e.close()


@pytest.mark.parametrize("level", [4, 3])
def test_straddling_tiles_with_several_records(level):
    """The geometry and launch pattern of test_gpu_18's test_waves_that_straddle_tiles_and_streams (n = 45 x 37 = 1 665 pixels per
    stream; odd frames go through one launch for stream 0 and one for streams 1 .. 2, whose waves start at 129, 193, ... inside a
    tile), with modes 12 levels apart: lanes on both sides of a tile boundary stream several records."""
    torch = _torch()
    S, H, W = 3, 45, 37
    T, n = 40, H * W
    s_min = _default_s_min()
    frames = np.stack([_banded(T, H, W, seed=11 * level + s, spacing=12) for s in range(S)], axis=1)
    eng = Engine(capi.MOG2, n_streams=S)
    eng.set_geometry(H, W, 3)
    eng.set_option(capi.OPT_MOG2_SPARSE, level)
    orcs = [pyoracle.Oracle(capi.MOG2) for _ in range(S)]
    d_fg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
    straddling_multi = 0
    for t in range(T):
        surv = np.concatenate([_survivors(orcs[s], frames[t, s], n, s_min, empty=t == 0)[0] for s in range(S)])  # by model pixel
        d = torch.from_numpy(frames[t]).cuda()
        if t % 2 == 0:
            assert eng.process_batch_device(d, d_fg, None, None) & capi.FG_VALID
        else:
            assert eng.process_batch_device(d[:1], d_fg[:1], None, None, first=0, count=1) & capi.FG_VALID
            assert eng.process_batch_device(d[1:], d_fg[1:], None, None, first=1, count=S - 1) & capi.FG_VALID
            for w0 in range(n, S * n, 64):  # the waves of the launch that starts at stream 1
                if w0 % 256 + 63 >= 256:
                    straddling_multi += int((surv[w0:min(w0 + 64, S * n)] >= 2).any())
        torch.cuda.synchronize()
        got = d_fg.cpu().numpy()
        for s in range(S):
            ofg, _ = orcs[s].process(frames[t, s], want_bg=False)
            assert np.array_equal(got[s], ofg), (level, t, s, int((got[s] != ofg).sum()))
    assert straddling_multi > 0
    for s in range(S):
        check_mog2_state(eng, orcs[s], n, stream=s)
        if level == 4:
            assert _mog2_summary_invariants(eng, n, stream=s) == 1.0
    eng.close()


_AUTO_PARTS = (80, 60, 60)
_AUTO_LEVEL = 130


def _auto_frames():
    """64 x 64.  80 frames of test_gpu_18's S_sat-like input (five modes 40 apart: one record of five survives), 60 frames of a single
    static level with noise +-2, 60 frames of five levels 6 apart around that level (every mode of a pixel ends up within 24 levels
    of every value: the summaries rule hardly anything out)."""
    H = W = 64
    rng = np.random.default_rng(6)
    first = _sat_like(_AUTO_PARTS[0], 1, H, W, seed=5)[:, 0]
    second = (_AUTO_LEVEL + rng.integers(-2, 3, (_AUTO_PARTS[1], H, W, 3))).astype(np.uint8)
    phase = rng.integers(0, 5, (H, W, 1))
    third = np.stack([(_AUTO_LEVEL + 6 * ((t + phase) % 5) + rng.integers(-2, 3, (H, W, 3))).astype(np.uint8) for t in range(_AUTO_PARTS[2])])
    return np.concatenate([first, second, third])


def _auto_child():
    """Runs in a child process with BGS_DEBUG_STAT set: auto mode over _auto_frames, parity on every frame, a marker on stderr
    between the parts (the library's own lines go to the C stderr, which is not buffered)."""
    torch = _torch()
    H = W = 64
    frames = _auto_frames()
    eng = Engine(capi.MOG2)
    eng.set_geometry(H, W, 3)
    eng.set_option(capi.OPT_MOG2_SPARSE, 3)
    orc = pyoracle.Oracle(capi.MOG2)
    d_fg = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    for t in range(len(frames)):
        if t in (_AUTO_PARTS[0], _AUTO_PARTS[0] + _AUTO_PARTS[1]):
            sys.stderr.write("[test] next part\n")
            sys.stderr.flush()
        assert eng.process_batch_device(torch.from_numpy(frames[t:t + 1]).cuda(), d_fg, None, None) & capi.FG_VALID
        torch.cuda.synchronize()
        ofg, _ = orc.process(frames[t], want_bg=False)
        got = d_fg[0].cpu().numpy()
        assert np.array_equal(got, ofg), (t, int((got != ofg).sum()))
    check_mog2_state(eng, orc, H * W)
    eng.close()
    print("parity on %d frames" % len(frames))


def test_auto_mode_still_decides_when_the_filter_kernel_samples_every_8th_launch():
    """Level 3 (auto).  The library prints every poll of the sampled counters when BGS_DEBUG_STAT is set ("... -> mode W (now N)").
    First part: the mode goes to 4.  Second part, the static level: the CPU side shows that the filter kernel KEEPS paying there - a
    pixel keeps its five modes (the reference never lowers the count), the static level creates one more in place of the weakest and
    leaves 2.2 records of 5 (0.43 of the live modes: below the rule's 0.5), so the mode correctly stays 4; what this part shows is the
    thinned sampling, 7 or 8 polls in 60 launches instead of 60.  Third part: levels 6 apart leave 0.6 of the live modes, the first
    poll that sees it brings back a sample on every launch, and the second one in a row leaves mode 4."""
    import re
    n = 64 * 64
    # the inputs reach those paths: on the oracle alone, before any GPU run
    s_min = _default_s_min()
    orc = pyoracle.Oracle(capi.MOG2)
    frac = []
    for t, f in enumerate(_auto_frames()):
        surv, nm = _survivors(orc, f, n, s_min, empty=t == 0)
        frac.append((float(surv.sum()) / max(1, int(nm.sum())), float(nm.mean()) / 5))
        orc.process(f, want_bg=False)
    a, b = _AUTO_PARTS[0], _AUTO_PARTS[0] + _AUTO_PARTS[1]
    assert all(nf < 0.35 and lf == 1.0 for nf, lf in frac[20:a])      # clear evidence for mode 4
    assert all(nf < 0.47 for nf, _ in frac[a:b])                       # still mode 4, with a margin to the rule's 0.5
    assert all(nf > 0.55 and lf == 1.0 for nf, lf in frac[b + 10:])   # mode 1, twice in a row
    env = dict(os.environ, BGS_DEBUG_STAT="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_19_mog2_stream as t; t._auto_child()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "parity on %d frames" % sum(_AUTO_PARTS) in r.stdout
    parts = r.stderr.split("[test] next part\n")
    assert len(parts) == 3, r.stderr[-2000:]
    polls = [[(int(w), int(now)) for w, now in re.findall(r"-> mode (\d) \(now (\d)\)", p)] for p in parts]
    print([len(p) for p in polls], polls)
    assert any(now == 4 for _, now in polls[0]), "the mode never went to 4 in the first part"
    assert polls[1] and all(now == 4 and want == 4 for want, now in polls[1]), polls[1]
    assert 6 <= len(polls[1]) <= 9, "60 filter launches in the steady state sample 7 or 8 times"
    assert polls[2][0][1] == 4 and any(now != 4 for _, now in polls[2]), "the mode did not leave 4 in the third part"

