"""bgs_group - several classes on the same frames (what FrameProcessor::process does with its pre-processed frame,
FrameProcessor.cpp:169-340): every output of a group must equal the oracle of its class and the separate engine of its class, bit for
bit - masks, backgrounds, warm-up conventions (outputs untouched), model states - whether the class runs inside the fused kernel or
as a member engine, on the host path and on the batched device path."""
import numpy as np
import pytest

from gpu_helpers import _params, _torch, check_mog2_state
from oracle import pyoracle
from tools import synth
from tracking_amd import Engine, capi
from tracking_amd.engine import Group

pytestmark = pytest.mark.gpu

FUSABLE = [capi.FRAME_DIFF, capi.STATIC_FRAME_DIFF, capi.WMM, capi.WMV, capi.ABL, capi.SIGMA_DELTA]


def _check_fused_state(grp, i, algo, orc, n):
    if algo in (capi.STATIC_FRAME_DIFF, capi.ABL):
        assert np.array_equal(grp.get_state(i, "bg", (n * 3,), np.uint8), orc.get_state("bg", (n * 3,), np.uint8)), (algo, "bg")
    if algo == capi.SIGMA_DELTA:
        for pl in ("mt", "vt"):
            assert np.array_equal(grp.get_state(i, pl, (n * 3,), np.uint8), orc.get_state(pl, (n * 3,), np.uint8)), pl


@pytest.mark.parametrize("algos", [FUSABLE, [capi.WMV, capi.ABL], [capi.FRAME_DIFF, capi.MOG2, capi.ABL, capi.ASBL],
                                   [capi.ABL, capi.ABL, capi.SIGMA_DELTA], [capi.WMM]])
@pytest.mark.parametrize("shape", [(48, 64), (37, 53)])
def test_group_host_path_equals_every_class_oracle(algos, shape, golden_frames):
    H, W = shape
    frames = np.ascontiguousarray(golden_frames[:14, :H, :W])
    grp = Group(algos)
    orcs = [pyoracle.Oracle(a) for a in algos]
    seen_first = set()
    for i, a in enumerate(algos):  # one instance of each byte-stream class is fused, everything else is a member engine
        assert grp.is_fused(i) == (a in FUSABLE and a not in seen_first), (i, a)
        seen_first.add(a)
    for t, f in enumerate(frames):
        outs = grp.process(f)
        for i, (a, orc) in enumerate(zip(algos, orcs)):
            ofg, obg = orc.process(f)
            fg, bg = outs[i]
            assert (fg is None) == (ofg is None), (t, i, a)
            assert (bg is None) == (obg is None), (t, i, a)
            if ofg is not None:
                assert np.array_equal(fg, ofg), (t, i, a, int((fg != ofg).sum()))
            if obg is not None:
                assert np.array_equal(bg.reshape(obg.shape), obg), (t, i, a)
    for i, (a, orc) in enumerate(zip(algos, orcs)):
        if grp.is_fused(i):
            _check_fused_state(grp, i, a, orc, H * W)
    assert grp.frames_seen() == len(frames)
    grp.close()


def test_group_parameter_changes_between_frames(golden_frames):
    """The wrappers re-read ./config/<Class>.xml on every process(): thresholds, weights and ABL's alpha (its 256 x 256 table is rebuilt)
    may change mid-stream, per class."""
    frames = golden_frames[:12]
    algos = [capi.WMV, capi.ABL, capi.FRAME_DIFF]
    grp = Group(algos)
    orcs = [pyoracle.Oracle(a) for a in algos]
    for t, f in enumerate(frames):
        if t == 5:
            pa, pw, pf = _params(capi.ABL, alpha=0.2, threshold=9), _params(capi.WMV, enable_weight=0, threshold=21), _params(capi.FRAME_DIFF, enable_threshold=0)
            for i, p in ((0, pw), (1, pa), (2, pf)):
                grp.set_params(i, p)
                orcs[i].set_params(p)
        outs = grp.process(f)
        for i, orc in enumerate(orcs):
            ofg, obg = orc.process(f)
            if ofg is not None:
                assert np.array_equal(outs[i][0], ofg), (t, i)
            else:
                assert outs[i][0] is None
            if obg is not None:
                assert np.array_equal(outs[i][1].reshape(obg.shape), obg), (t, i)
    grp.close()


@pytest.mark.parametrize("borrow", [False, True])
def test_group_device_batch_equals_separate_engines_and_oracles(borrow):
    """Batched device path, 3 streams: the fused kernel's outputs against separate engines of each class (same device frames) and
    against one oracle per stream and class; warm-up frames leave the outputs untouched."""
    torch = _torch()
    S, T, H, W = 3, 9, 32, 64
    algos = [capi.FRAME_DIFF, capi.STATIC_FRAME_DIFF, capi.WMM, capi.WMV, capi.ABL, capi.SIGMA_DELTA, capi.MOG2]
    clips = np.stack([synth.random_frames(T, H, W, 3, seed=300 + s) for s in range(S)])
    grp = Group(algos, n_streams=S)
    grp.set_geometry(H, W, 3)
    if borrow:
        grp.set_option(capi.OPT_BORROW_FRAMES, 1)
    engs = [Engine(a, n_streams=S) for a in algos]
    for e in engs:
        e.set_geometry(H, W, 3)
    orcs = [[pyoracle.Oracle(a) for _ in range(S)] for a in algos]
    keep = []
    for t in range(T):
        d_frames = torch.from_numpy(np.ascontiguousarray(clips[:, t])).cuda()
        keep.append(d_frames)  # borrowed history must stay alive
        fgs = [torch.full((S, H, W), 9, dtype=torch.uint8, device="cuda") for _ in algos]
        bgs_ = [torch.full((S, H, W, 3), 9, dtype=torch.uint8, device="cuda") for _ in algos]
        flags = grp.process_batch_device(d_frames, fgs, bgs_)
        torch.cuda.synchronize()
        for i, a in enumerate(algos):
            efg = torch.full((S, H, W), 9, dtype=torch.uint8, device="cuda")
            ebg = torch.full((S, H, W, 3), 9, dtype=torch.uint8, device="cuda")
            efl = engs[i].process_batch_device(d_frames, efg, ebg, None)
            torch.cuda.synchronize()
            assert flags[i] == efl, (t, i, a, flags[i], efl)
            assert torch.equal(fgs[i], efg), (t, i, a, "mask vs separate engine")
            assert torch.equal(bgs_[i], ebg), (t, i, a, "background vs separate engine")
            for s in range(S):
                ofg, obg = orcs[i][s].process(clips[s, t])
                assert bool(flags[i] & capi.FG_VALID) == (ofg is not None) and bool(flags[i] & capi.BG_VALID) == (obg is not None), (t, i, s)
                if ofg is not None:
                    assert np.array_equal(fgs[i][s].cpu().numpy(), ofg), (t, i, a, s)
                if obg is not None:
                    assert np.array_equal(bgs_[i][s].cpu().numpy().reshape(obg.shape), obg), (t, i, a, s)
    for s in range(S):
        check_mog2_state(engs[6], orcs[6][s], H * W, stream=s)
        mog2 = [grp.get_state(6, pl, sh, np.float32, stream=s) for pl, sh in (("w", (5, H * W)), ("var", (5, H * W)), ("mu", (5, 3, H * W)))]
        ref = [engs[6].get_state(pl, sh, np.float32, stream=s) for pl, sh in (("w", (5, H * W)), ("var", (5, H * W)), ("mu", (5, 3, H * W)))]
        assert all(np.array_equal(a, b) for a, b in zip(mog2, ref)), "member engine state"
    grp.close()


def test_group_config2_full_size_wmv_abl_sampled_parity():
    """BASELINE configs[2] as one fused launch: WeightedMovingVarianceBGS + AdaptiveBackgroundLearning on the same 3840x2160 frames,
    borrowed history (17 B/pixel).  Every pixel against the two separate engines; a band of rows of each against the oracles."""
    torch = _torch()
    H, W, T = 2160, 3840, 5
    frames = synth.s_surv(T, H, W, seed=77, device="cuda")
    grp = Group([capi.WMV, capi.ABL])
    grp.set_geometry(H, W, 3)
    grp.set_option(capi.OPT_BORROW_FRAMES, 1)
    ew, ea = Engine(capi.WMV), Engine(capi.ABL)
    for e in (ew, ea):
        e.set_geometry(H, W, 3)
    ew.set_option(capi.OPT_BORROW_FRAMES, 1)
    y0, y1 = 1000, 1064
    ow, oa = pyoracle.Oracle(capi.WMV), pyoracle.Oracle(capi.ABL)
    for t in range(T):
        fr = frames[t:t + 1]
        fgs = [torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda") for _ in range(2)]
        bg = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda")
        fl = grp.process_batch_device(fr, fgs, [None, bg])
        f1 = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        f2 = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        b2 = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda")
        assert fl[0] == ew.process_batch_device(fr, f1, None, None) and fl[1] == ea.process_batch_device(fr, f2, b2, None)
        torch.cuda.synchronize()
        assert torch.equal(fgs[0], f1) and torch.equal(fgs[1], f2) and torch.equal(bg, b2), t
        band = np.ascontiguousarray(frames[t, y0:y1].cpu().numpy())
        wfg, _ = ow.process(band)
        afg, abg = oa.process(band)
        if wfg is not None:
            assert np.array_equal(fgs[0][0, y0:y1].cpu().numpy(), wfg), t
        assert np.array_equal(fgs[1][0, y0:y1].cpu().numpy(), afg) and np.array_equal(bg[0, y0:y1].cpu().numpy(), abg), t
    grp.close()


def test_group_argument_errors():
    with pytest.raises(capi.BgsError):
        Group([capi.SIGMA_DELTA, capi.ABL]).process(np.zeros((8, 8), np.uint8))  # SigmaDelta is 3-channel only
    g = Group([capi.WMV, capi.ABL], n_streams=2)
    with pytest.raises(capi.BgsError):
        g.process(np.zeros((8, 8, 3), np.uint8))  # the host call serves single-stream groups
    g.close()
    g = Group([capi.FRAME_DIFF, capi.WMV])
    g.process(np.zeros((8, 16, 3), np.uint8))
    with pytest.raises(capi.BgsError):
        g.process(np.zeros((9, 16, 3), np.uint8))  # a group keeps its geometry
    g.close()


# ---- the state a group shares with the separate engines of its fused classes: the frame history ring, ABL's update rule and table,
# SigmaDelta's first frame, the launch timer ----------------------------------------------------------------------------------------

RING = [capi.FRAME_DIFF, capi.WMM, capi.WMV]


def _refused(call, code=capi.ERR_STATE):
    with pytest.raises(capi.BgsError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def _check_history_planes(get, given, depth, what):
    """given: the frames the stream has been fed since its (re)start, oldest first; depth: frames of history the ring keeps"""
    for k, plane in ((1, "prev1"), (2, "prev2")):
        if len(given) >= k and k <= depth:
            assert np.array_equal(get(plane), given[-k].reshape(-1)), (what, plane, len(given))
        else:
            _refused(lambda: get(plane))


@pytest.mark.parametrize("shape", [(37, 53), (32, 64)])
def test_history_planes_are_the_last_two_frames_of_each_stream(shape):
    """`prev1` / `prev2` after every frame: the last and the last but one frame the stream was fed, byte for byte, refused
    (BGS_ERR_STATE) while that frame does not exist.  Separate engines (stream 1 is reset before frame 3: its planes follow its own age
    while the others go on; FrameDifference keeps one frame, so its `prev2` is always refused), a group of all three (one shared ring
    of three slots, which also answers FrameDifference's `prev2`), a group of FrameDifference alone (two slots) and a group with
    BGS_OPT_BORROW_FRAMES, which refuses both planes."""
    torch = _torch()
    (H, W), S, T = shape, 3, 5
    nb = H * W * 3
    clips = np.stack([synth.random_frames(T, H, W, 3, seed=500 + s) for s in range(S)])
    grp, grp_fd, grp_borrow = Group(RING, n_streams=S), Group([capi.FRAME_DIFF], n_streams=S), Group(RING, n_streams=S)
    grp_borrow.set_option(capi.OPT_BORROW_FRAMES, 1)
    engs = [Engine(a, n_streams=S) for a in RING]
    for x in [grp, grp_fd, grp_borrow] + engs:
        x.set_geometry(H, W, 3)
    fed_e, fed_g = [[] for _ in range(S)], [[] for _ in range(S)]

    def check_all():
        for s in range(S):
            for i, a in enumerate(RING):
                _check_history_planes(lambda pl: engs[i].get_state(pl, (nb,), np.uint8, stream=s), fed_e[s], 1 if a == capi.FRAME_DIFF else 2, ("engine", a, s))
                _check_history_planes(lambda pl: grp.get_state(i, pl, (nb,), np.uint8, stream=s), fed_g[s], 2, ("group", a, s))
                _check_history_planes(lambda pl: grp_borrow.get_state(i, pl, (nb,), np.uint8, stream=s), fed_g[s], 0, ("borrowing group", a, s))
            _check_history_planes(lambda pl: grp_fd.get_state(0, pl, (nb,), np.uint8, stream=s), fed_g[s], 1, ("group of FrameDifference", s))

    check_all()
    keep = []
    for t in range(T):
        if t == 3:
            for e in engs:
                e.reset_stream(1)
            fed_e[1] = []
        d_frames = torch.from_numpy(np.ascontiguousarray(clips[:, t])).cuda()
        keep.append(d_frames)  # borrowed history must stay alive
        for g in (grp, grp_fd, grp_borrow):
            n = len(g.algos)
            g.process_batch_device(d_frames, [torch.empty((S, H, W), dtype=torch.uint8, device="cuda") for _ in range(n)],
                                   [torch.empty((S, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(n)])
        for e in engs:
            e.process_batch_device(d_frames, torch.empty((S, H, W), dtype=torch.uint8, device="cuda"), torch.empty((S, H, W, 3), dtype=torch.uint8, device="cuda"), None)
        torch.cuda.synchronize()
        for s in range(S):
            fed_e[s].append(clips[s, t]), fed_g[s].append(clips[s, t])
        check_all()
    for x in [grp, grp_fd, grp_borrow] + engs:
        x.close()


@pytest.mark.parametrize("limit", [-1, 0, 3])
def test_group_abl_update_rule_and_table_equal_engine_and_oracle(limit, golden_frames):
    """AdaptiveBackgroundLearning fused (class 0) and as a member engine (class 1) side by side, against the separate engine and the
    oracle: `limit` -1 (always learn), 0 and 3 (the reference's counter never passes a positive limit), alpha changed at frame 4 (the
    table is rebuilt).  Masks, backgrounds and the `bg` plane after every frame."""
    H, W = 37, 53
    frames = np.ascontiguousarray(golden_frames[:9, :H, :W])
    p = _params(capi.ABL, limit=limit)
    grp = Group([capi.ABL, capi.ABL], params=[_params(capi.ABL, limit=limit), _params(capi.ABL, limit=limit)])
    assert grp.is_fused(0) and not grp.is_fused(1)
    eng, orc = Engine(capi.ABL, params=p), pyoracle.Oracle(capi.ABL, params=p)
    for t, f in enumerate(frames):
        if t == 4:
            for i in range(2):
                grp.set_params(i, _params(capi.ABL, limit=limit, alpha=0.2))
            eng.set_params(_params(capi.ABL, limit=limit, alpha=0.2))
            orc.set_params(_params(capi.ABL, limit=limit, alpha=0.2))
        outs = grp.process(f)
        efg, ebg = eng.process(f)
        ofg, obg = orc.process(f)
        state = orc.get_state("bg", (H * W * 3,), np.uint8)
        assert np.array_equal(efg, ofg) and np.array_equal(ebg.reshape(obg.shape), obg), (t, "engine")
        assert np.array_equal(eng.get_state("bg", (H * W * 3,), np.uint8), state), (t, "engine bg plane")
        for i in range(2):
            assert np.array_equal(outs[i][0], ofg), (t, i, "mask")
            assert np.array_equal(outs[i][1].reshape(obg.shape), obg), (t, i, "background")
            assert np.array_equal(grp.get_state(i, "bg", (H * W * 3,), np.uint8), state), (t, i, "bg plane")
    grp.close(), eng.close()


def test_group_fused_sigmadelta_planes_and_geometry_refusal(golden_frames):
    """A fused SigmaDelta answers `mt` and `vt` from its first frame on (refused before it) and never `bg`; a 1-channel group that
    holds it is refused with the separate engine's code and text."""
    H, W = 37, 53
    frames = np.ascontiguousarray(golden_frames[:4, :H, :W])
    grp, orc = Group([capi.SIGMA_DELTA, capi.ABL]), pyoracle.Oracle(capi.SIGMA_DELTA)
    assert grp.is_fused(0)
    grp.set_geometry(H, W, 3)
    for pl in ("mt", "vt", "bg"):
        _refused(lambda: grp.get_state(0, pl, (H * W * 3,), np.uint8))
    for t, f in enumerate(frames):
        outs = grp.process(f)
        ofg, _ = orc.process(f)
        assert (outs[0][0] is None) == (ofg is None) and (ofg is None or np.array_equal(outs[0][0], ofg)), t
        for pl in ("mt", "vt"):
            assert np.array_equal(grp.get_state(0, pl, (H * W * 3,), np.uint8), orc.get_state(pl, (H * W * 3,), np.uint8)), (t, pl)
        _refused(lambda: grp.get_state(0, "bg", (H * W * 3,), np.uint8))
    grp.close()
    eng, gray = Engine(capi.SIGMA_DELTA), Group([capi.WMV, capi.SIGMA_DELTA])
    text = _refused(lambda: eng.set_geometry(8, 8, 1), capi.ERR_UNSUPPORTED)
    assert _refused(lambda: gray.set_geometry(8, 8, 1), capi.ERR_UNSUPPORTED) == text and "3-channel only" in text
    gray.set_geometry(8, 8, 3)  # the refusal left no geometry behind
    eng.close(), gray.close()


def test_kernel_timing_counts_launches_of_group_and_engine(golden_frames):
    """One timed pair per fused launch of a group (every frame launches: ABL has no warm-up) and per launch of an engine
    (FrameDifference's first frame launches nothing); enabling timing again drops what was recorded."""
    frames = np.ascontiguousarray(golden_frames[:5, :37, :53])
    grp, eng = Group([capi.WMV, capi.ABL]), Engine(capi.FRAME_DIFF)
    grp.enable_kernel_timing(), eng.enable_kernel_timing()
    for f in frames:
        grp.process(f), eng.process(f)
    ms, n = grp.kernel_timing()
    assert n == 5 and ms > 0, (ms, n)
    ms, n, name = eng.kernel_timing()
    assert n == 4 and ms > 0 and name == "framediff_kernel", (ms, n, name)
    assert len(eng.kernel_timing_series()) == 4
    grp.enable_kernel_timing(), eng.enable_kernel_timing()
    assert grp.kernel_timing() == (0.0, 0) and eng.kernel_timing()[:2] == (0.0, 0)
    grp.close(), eng.close()


def test_ring_class_clip_then_host_path_then_submit():
    """WeightedMovingMean: a 5-frame clip call (the clip's own frames are its history; the ring is brought up to date at the end), then
    two bgs_process frames, then two bgs_submit / bgs_wait frames (both upload straight into the ring slot): masks and backgrounds of
    the oracle's 9-frame run, and the history planes are the last two frames after the clip and at the end."""
    torch = _torch()
    H, W, T = 48, 64, 9
    clip = synth.random_frames(T, H, W, 3, seed=77)
    eng, orc = Engine(capi.WMM), pyoracle.Oracle(capi.WMM)
    eng.set_geometry(H, W, 3)
    ref = [orc.process(f) for f in clip]

    def check_planes(t):  # after frames 0..t
        for k, pl in ((1, "prev1"), (2, "prev2")):
            assert np.array_equal(eng.get_state(pl, (H * W * 3,), np.uint8), clip[t + 1 - k].reshape(-1)), (t, pl)

    d_fg = torch.full((5, 1, H, W), 9, dtype=torch.uint8, device="cuda")
    d_bg = torch.full((5, 1, H, W, 3), 9, dtype=torch.uint8, device="cuda")
    d_frames = torch.from_numpy(np.ascontiguousarray(clip[:5].reshape(5, 1, H, W, 3))).cuda()
    flags = eng.process_clip_device(d_frames, 5, d_fg, d_bg)
    torch.cuda.synchronize()
    for t in range(5):
        ofg, obg = ref[t]
        assert flags[t] == (0 if ofg is None else capi.FG_VALID | capi.BG_VALID), t
        if ofg is None:
            assert (d_fg[t] == 9).all() and (d_bg[t] == 9).all(), t
        else:
            assert np.array_equal(d_fg[t, 0].cpu().numpy(), ofg) and np.array_equal(d_bg[t, 0].cpu().numpy(), obg), t
    check_planes(4)
    for t in (5, 6):
        fg, bg = eng.process(clip[t])
        assert np.array_equal(fg, ref[t][0]) and np.array_equal(bg, ref[t][1]), t
    for t in (7, 8):
        fg, bg = np.empty((H, W), np.uint8), np.empty((H, W, 3), np.uint8)
        eng.submit(clip[t], fg, bg)
        assert eng.wait() == capi.FG_VALID | capi.BG_VALID
        assert np.array_equal(fg, ref[t][0]) and np.array_equal(bg, ref[t][1]), t
    check_planes(8)
    assert np.array_equal(eng.get_state("prev1", (H * W * 3,), np.uint8), orc.get_state("prev1", (H * W * 3,), np.uint8))
    assert np.array_equal(eng.get_state("prev2", (H * W * 3,), np.uint8), orc.get_state("prev2", (H * W * 3,), np.uint8))
    eng.close()
