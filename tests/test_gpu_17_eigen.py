"""DPEigenbackgroundBGS (BGS_DP_EIGENBACKGROUND, USTC_BGS type 15's class) on the GPU against the outputs of the reference's own
dp/Eigenbackground.cpp (tests/golden/eigen_ref.npz, read through tests/eigen_numpy.py; nothing here needs the reference tree) and
against the float64 restatement that tests/test_eigen_cpu.py holds to that fixture.

The PCA is pinned as mathematics: `result` within TOL_RESULT of the restatement, eigenvalues within 1e-9 of the
largest one, eigenvectors within 1e-5 of parallel, masks equal outside the near-threshold band.  Everything around it is exact: the
learning frames, the history bytes, avg, the `static` case, and every path against the host path, byte for byte."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import eigen_numpy as en
from gpu_helpers import _torch
from tracking_amd import Engine, capi, node

pytestmark = pytest.mark.gpu

ALGO = capi.DP_EIGENBACKGROUND
PKEYS = ("threshold", "history_size", "embedded_dim")
PLANES = (("avg", np.float32), ("eigenvalues", np.float64), ("eigenvectors", np.float32), ("coeff", np.float32), ("result", np.float32))


def engine(p, n_streams=1):
    e = Engine(ALGO, n_streams=n_streams)
    e.set_eigen_params(**{k: p[k] for k in PKEYS})
    return e


def plane_shape(plane, p, n):
    return {"avg": (n * 3,), "eigenvalues": (p["history_size"],), "eigenvectors": (p["embedded_dim"], n * 3), "coeff": (p["embedded_dim"],), "result": (n * 3,),
            "history": (p["history_size"], n * 3)}[plane]


def state_of(eng, p, n, stream=0):
    """Every plane of a stream that has detected, as bytes."""
    out = {pl: eng.get_state(pl, plane_shape(pl, p, n), dt, stream=stream) for pl, dt in PLANES}
    out["history"] = eng.get_state("history", plane_shape("history", p, n), np.uint8, stream=stream)
    return out


def same_state(a, b, where):
    for pl in a:
        assert a[pl].tobytes() == b[pl].tobytes(), (where, pl)


@functools.lru_cache(maxsize=None)
def restated(case):
    r = en.load()[case]
    masks, results, mdl = en.run(r["params"], r["frames"])
    for a in (masks, results):
        a.setflags(write=False)
    return masks, results, mdl


@functools.lru_cache(maxsize=None)
def single(case):
    """The host path on a fixture case, one stream: masks [T][H][W] and the state after the last frame.  Computed once; every other
    path is compared with it byte for byte."""
    r = en.load()[case]
    frames, p = r["frames"], r["params"]
    eng = engine(p)
    masks = []
    for f in frames:
        fg, bg = eng.process(f, want_bg=True)
        assert bg is None and fg is not None  # BGS_FG_VALID from frame 0, BGS_BG_VALID never
        masks.append(fg)
    st = state_of(eng, p, frames.shape[1] * frames.shape[2])
    eng.close()
    masks = np.array(masks)
    masks.setflags(write=False)
    return masks, st


def words_of(mask, Wd):
    packed = np.packbits(mask.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
    w = np.zeros(Wd * 8, np.uint8)
    w[:len(packed)] = packed
    return w.view(np.uint64)


def check_against_restatement(p, frames, masks, st, mdl, results, where, want_masks=None):
    """masks outside the band, result, eigenvalues, eigenvectors against the float64 restatement (and the fixture's masks)."""
    Hs, M = p["history_size"], p["embedded_dim"]
    T = len(frames)
    assert not masks[:Hs].any(), (where, "learning frames")
    assert st["history"].tobytes() == frames[:Hs].tobytes(), (where, "history")
    for k, t in enumerate(range(Hs, T)):
        near = en.band(p, frames[t], results[k])
        for name, want in (("restatement", None), ("fixture", want_masks)):
            w = (np.where((((frames[t].reshape(-1).astype(np.float64) - results[k]) ** 2) > np.float64(en.thresholds(p)[1])).reshape(-1, 3).any(1), 255, 0)
                 if want is None else want[t].reshape(-1))
            bad = (masks[t].reshape(-1) != w) & ~near
            assert not bad.any(), (where, name, t, int(bad.sum()))
    diff = float(np.abs(st["result"].astype(np.float64) - results[-1]).max())
    print("%s: largest |result - r64| %.3g (TOL_RESULT %.3g)" % (where, diff, en.TOL_RESULT))
    assert diff <= en.TOL_RESULT, (where, diff)
    lam = mdl.lam
    assert np.abs(st["eigenvalues"] - lam).max() <= 1e-9 * max(lam[0], 1e-300), (where, st["eigenvalues"], lam)
    assert (np.diff(st["eigenvalues"]) <= 0).all(), (where, "descending")
    E, Er = st["eigenvectors"].astype(np.float64), mdl.E.astype(np.float64)
    for i in range(M):
        if not Er[i].any():
            assert not E[i].any(), (where, "row %d must be zero" % i)  # the zero-row rule
        else:
            c = abs(float(E[i] @ Er[i])) / np.sqrt(float(E[i] @ E[i]) * float(Er[i] @ Er[i]))
            assert c >= 1 - 1e-5, (where, i, c)
    S = mdl.history.astype(np.int64).sum(0)
    assert st["avg"].tobytes() == (S.astype(np.float32) / np.float32(Hs)).tobytes(), (where, "avg")


@pytest.mark.parametrize("case", list(en.cases()))
def test_host_path_matches_reference_fixture(case):
    r = en.load()[case]
    frames, p = r["frames"], r["params"]
    masks, st = single(case)
    _, results, mdl = restated(case)
    if case == "static":  # exact: Gc = 0, every row zero, result = avg = the bytes
        assert np.array_equal(masks, r["masks"])
        assert not st["eigenvectors"].any() and not st["eigenvalues"].any() and not st["coeff"].any()
        assert st["result"].tobytes() == st["avg"].tobytes() == frames[0].reshape(-1).astype(np.float32).tobytes()
        assert st["result"].tobytes() == r["result"].tobytes() and st["avg"].tobytes() == r["avg"].tobytes()
        return
    if case in en.NO_PARITY:  # rank below M: the zero-row rule against the restatement; not a parity claim
        rank = int((mdl.E != 0).any(1).sum())
        assert rank < p["embedded_dim"] and not st["eigenvectors"][rank:].any()
        check_against_restatement(p, frames, masks, st, mdl, results, case)
        return
    check_against_restatement(p, frames, masks, st, mdl, results, case, want_masks=r["masks"])
    if "avg" in r:
        assert st["avg"].tobytes() == r["avg"].tobytes()
        assert np.abs(st["result"].astype(np.float64) - r["result"].astype(np.float64)).max() <= 2 * en.TOL_RESULT
        assert np.abs(st["eigenvalues"] - r["eigenvalues"]).max() <= 1e-9 * r["eigenvalues"][0]


def test_batch_path_streams_in_different_phases_equal_their_single_stream_runs():
    """Three streams of 37 x 53 in one engine; stream k joins 2 k steps late, so a launch mixes learning, building and detecting
    streams (three runs) and later covers all three at once: masks, packed words and the final state of every stream equal its
    single-stream host run byte for byte - a stream's chunking depends on its own n alone."""
    torch = _torch()
    cases = ("ragged", "ragged_o1", "ragged_o2")
    rs = [en.load()[c] for c in cases]
    T, H, W = rs[0]["masks"].shape
    n, Wd, S = H * W, (H * W + 63) // 64, 3
    p = rs[0]["params"]
    eng = engine(p, n_streams=S)
    eng.set_geometry(H, W, 3)
    start = [0, 2, 4]
    for u in range(T):
        k = sum(1 for s in range(S) if start[s] <= u)
        d_frames = torch.from_numpy(np.stack([rs[s]["frames"][u - start[s]] for s in range(k)])).cuda()
        d_fg = torch.full((k, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((k, Wd), -1, dtype=torch.int64, device="cuda")
        assert eng.process_batch_device(d_frames, d_fg, None, d_bits, first=0, count=k) == capi.FG_VALID
        torch.cuda.synchronize()
        fg, bits = d_fg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
        for s in range(k):
            want = single(cases[s])[0][u - start[s]]
            assert np.array_equal(fg[s], want), (u, s, int((fg[s] != want).sum()))
            assert np.array_equal(bits[s], words_of(want, Wd)), (u, s)
    assert [eng.frames_seen(s) for s in range(S)] == [T - start[s] for s in range(S)]
    same_state(state_of(eng, p, n, stream=0), single("ragged")[1], "stream 0")
    for s in (1, 2):  # their clips have not ended: model planes equal (the model never changes), coeff / result are of another frame
        st, want = state_of(eng, p, n, stream=s), single(cases[s])[1]
        for pl in ("avg", "eigenvalues", "eigenvectors", "history"):
            assert st[pl].tobytes() == want[pl].tobytes(), (s, pl)
    eng.close()


def test_node_step_equals_the_single_stream_runs():
    """The same three streams through bgs_node (one device, lock-step): the gathered packed masks equal each stream's own run."""
    torch = _torch()
    cases = ("ragged", "ragged_o1", "ragged_o2")
    rs = [en.load()[c] for c in cases]
    T, H, W = rs[0]["masks"].shape
    n, S = H * W, 3
    nd = node.Node(ALGO, S, devices=[0], transport=node.RCCL, flags=0)
    nd.set_geometry(H, W, 3)
    out = torch.empty((S, nd.words_per_stream), dtype=torch.int64, device="cuda")
    for t in range(T):
        flags = nd.step_device([torch.from_numpy(np.stack([r["frames"][t] for r in rs])).cuda()])
        nd.copy_masks(out)
        torch.cuda.synchronize()
        assert flags & capi.FG_VALID
        bits = out.cpu().numpy().view(np.uint64)
        for s in range(S):
            assert np.array_equal(bits[s], words_of(single(cases[s])[0][t], nd.words_per_stream)), (t, s)
    nd.sync()
    nd.close()


@pytest.mark.parametrize("case", ["tile", "ragged"])
@pytest.mark.parametrize("T", [2, 4, 8])
def test_clip_straddling_the_build_frame_equals_the_host_path(case, T):
    """Frames 0 .. H-2 one by one, then clips of T frames to the end: the first clip holds the last learning frame, the frame that
    builds the model and detecting frames.  Masks, packed words and the final state equal the host path's byte for byte; a second
    engine given the same calls gives the same bytes (no float atomics: run-to-run reproducible)."""
    torch = _torch()
    r = en.load()[case]
    frames, p = r["frames"], r["params"]
    N, H, W = frames.shape[:3]
    n, Wd, Hs = H * W, (H * W + 63) // 64, p["history_size"]
    want_masks, want_state = single(case)
    d_all = torch.from_numpy(np.array(frames)).cuda().unsqueeze(1)  # [N][1][H][W][3]
    states = []
    for _ in range(2):
        eng = engine(p)
        eng.set_geometry(H, W, 3)
        fg = np.empty((N, H, W), np.uint8)
        bits = np.empty((N, Wd), np.uint64)
        t = 0
        while t < N:
            k = 1 if t < Hs - 1 else min(T, N - t)
            d_fg = torch.full((k, 1, H, W), 9, dtype=torch.uint8, device="cuda")
            d_bits = torch.full((k, 1, Wd), -1, dtype=torch.int64, device="cuda")
            assert eng.process_clip_device(d_all[t:t + k], k, d_fg, None, d_bits) == [capi.FG_VALID] * k
            torch.cuda.synchronize()
            fg[t:t + k], bits[t:t + k] = d_fg.cpu().numpy()[:, 0], d_bits.cpu().numpy().view(np.uint64)[:, 0]
            t += k
        assert np.array_equal(fg, want_masks), int((fg != want_masks).sum())
        for t in range(N):
            assert np.array_equal(bits[t], words_of(want_masks[t], Wd)), t
        states.append(state_of(eng, p, n))
        eng.close()
    same_state(states[0], want_state, "clip against the host path")
    same_state(states[0], states[1], "two runs of the same clip")


@pytest.mark.parametrize("case", ["tile", "ragged"])
def test_range_path_and_submit_wait_equal_the_host_path(case):
    torch = _torch()
    r = en.load()[case]
    frames, p = r["frames"], r["params"]
    N, H, W = frames.shape[:3]
    n, Wd = H * W, (H * W + 63) // 64
    want_masks, want_state = single(case)
    rng_eng, sub_eng = engine(p, n_streams=2), engine(p, n_streams=2)
    rng_eng.set_geometry(H, W, 3)
    fg = np.empty((H, W), np.uint8)
    for t in range(N):
        d_fg = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        assert rng_eng.process_batch_device(torch.from_numpy(np.array(frames[t][None])).cuda(), d_fg, None, None, first=1, count=1) == capi.FG_VALID  # stream 1 alone
        torch.cuda.synchronize()
        assert np.array_equal(d_fg.cpu().numpy()[0], want_masks[t]), ("range", t)
        sub_eng.submit(np.ascontiguousarray(frames[t]), fg, None, stream=1)
        assert sub_eng.wait(stream=1) == capi.FG_VALID
        assert np.array_equal(fg, want_masks[t]), ("submit", t)
    same_state(state_of(rng_eng, p, n, stream=1), want_state, "range")
    same_state(state_of(sub_eng, p, n, stream=1), want_state, "submit / wait")
    assert rng_eng.frames_seen(0) == 0 and rng_eng.frames_seen(1) == N
    rng_eng.close(), sub_eng.close()


def test_reset_stream_restarts_the_history_and_leaves_the_other_stream_alone():
    """h8_m3 on two streams; stream 0 is reset while detecting (step 10) and fed its clip again from frame 0: its history restarts
    (slots beyond the frames seen read 0), stream 1 goes on unchanged, and the rebuilt model equals a fresh engine's."""
    torch = _torch()
    r = en.load()["h8_m3"]
    frames, p = r["frames"], r["params"]
    N, H, W = frames.shape[:3]
    n, Hs = H * W, p["history_size"]
    want_masks, want_state = single("h8_m3")
    eng = engine(p, n_streams=2)
    eng.set_geometry(H, W, 3)
    reset_at = 10
    for u in range(reset_at + N):
        if u == reset_at:
            eng.reset_stream(0)
            assert eng.frames_seen(0) == 0 and eng.frames_seen(1) == reset_at
            with pytest.raises(capi.BgsError):
                eng.get_state("avg", (n * 3,), np.float32, stream=0)  # no model yet
        t0 = u if u < reset_at else u - reset_at
        live = [0, 1] if u < N else [0]
        d_frames = torch.from_numpy(np.stack([frames[t0] if s == 0 else frames[u] for s in live])).cuda()
        d_fg = torch.full((len(live), H, W), 9, dtype=torch.uint8, device="cuda")
        assert eng.process_batch_device(d_frames, d_fg, None, None, first=0, count=len(live)) == capi.FG_VALID
        torch.cuda.synchronize()
        fg = d_fg.cpu().numpy()
        assert np.array_equal(fg[0], want_masks[t0]), (u, "stream 0")
        if 1 in live:
            assert np.array_equal(fg[1], want_masks[u]), (u, "stream 1")
        if u == reset_at + 1:
            hist = eng.get_state("history", (Hs, n * 3), np.uint8, stream=0)
            assert hist[:2].tobytes() == frames[:2].tobytes() and not hist[2:].any()
    same_state(state_of(eng, p, n, stream=0), want_state, "stream 0 after its reset")
    same_state(state_of(eng, p, n, stream=1), want_state, "stream 1")
    eng.close()


def test_bright_frames_do_not_wrap_a_32_bit_gram_sum():
    """150 x 150, every byte >= 250, H 4, M 2: 3 n = 67 500 elements of at least 62 500 each sum past 2^32.  Eigenvalues and avg
    against the restatement's exact integer Gram matrix."""
    rng = np.random.default_rng(77)
    p = dict(threshold=225, history_size=4, embedded_dim=2)
    frames = rng.integers(250, 256, (5, 150, 150, 3)).astype(np.uint8)
    assert int((frames[0].astype(np.int64) ** 2).sum()) > 1 << 32
    _, _, mdl = en.run(p, frames)
    eng = engine(p)
    for f in frames:
        eng.process(f, want_bg=False)
    lam = eng.get_state("eigenvalues", (4,), np.float64)
    avg = eng.get_state("avg", (67500,), np.float32)
    eng.close()
    assert np.abs(lam - mdl.lam).max() <= 1e-9 * mdl.lam[0], (lam, mdl.lam)
    assert avg.tobytes() == (mdl.history.astype(np.int64).sum(0).astype(np.float32) / np.float32(4)).tobytes()


def test_one_stream_at_1080p():
    """1920 x 1080, H 4, M 2, 6 frames: chunk indexing and 64-bit sums at the workload's size.  The clip is a 135 x 240 seeded clip
    enlarged 8 x (the same low-rank structure), with a bright box in the two detecting frames."""
    small = en.pca_clip(6, 135, 240, 31, quiet=99)
    frames = np.repeat(np.repeat(small, 8, axis=1), 8, axis=2)
    frames[4:, 300:500, 700:1000] = np.minimum(frames[4:, 300:500, 700:1000].astype(np.int16) + 90, 255).astype(np.uint8)
    p = dict(threshold=225, history_size=4, embedded_dim=2)
    masks, results, mdl = en.run(p, frames)
    assert mdl.lam[1] / mdl.lam[2] >= en.EIGENGAP
    eng = engine(p)
    got = np.array([eng.process(f, want_bg=False)[0] for f in frames])
    n = 1080 * 1920
    res = eng.get_state("result", (n * 3,), np.float32)
    eng.close()
    diff = float(np.abs(res.astype(np.float64) - results[-1]).max())
    print("1080p: largest |result - r64| %.3g (TOL_RESULT %.3g)" % (diff, en.TOL_RESULT))
    assert diff <= en.TOL_RESULT
    assert not got[:4].any()
    for k, t in enumerate((4, 5)):
        near = en.band(p, frames[t], results[k])
        assert near.mean() <= en.BAND_SHARE
        bad = (got[t].reshape(-1) != masks[t].reshape(-1)) & ~near
        assert not bad.any(), (t, int(bad.sum()))
        assert (got[t] != 0).sum() >= 20000


def test_parameters_set_after_the_geometry_leave_the_values_in_force():
    r = en.load()["h8_m3"]
    frames, p = r["frames"], r["params"]
    eng = engine(p)
    for t, f in enumerate(frames):
        if t == 3:
            eng.set_eigen_params(threshold=1, history_size=5, embedded_dim=4)  # accepted, changes nothing
            with pytest.raises(capi.BgsError):  # a refusal stays a refusal
                eng.set_eigen_params(history_size=33)
        fg, _ = eng.process(f, want_bg=False)
        assert np.array_equal(fg, single("h8_m3")[0][t]), t
    q = eng.get_eigen_params()
    assert (q.threshold, q.history_size, q.embedded_dim) == (p["threshold"], p["history_size"], p["embedded_dim"])
    eng.close()


def test_no_background_gray_frames_refused_and_params_of_other_classes():
    eng = Engine(ALGO)
    with pytest.raises(capi.BgsError) as ei:
        eng.process(np.zeros((12, 16), np.uint8))
    assert ei.value.code == capi.ERR_UNSUPPORTED and en.CLASS_NAME in str(ei.value)
    for t in range(23):  # still usable; the defaults: 20 learning frames, then detection
        fg, bg = eng.process(np.full((4, 4, 3), 7 * t, np.uint8))
        assert bg is None and fg is not None and not (eng.stream_flags(0) & capi.BG_VALID)
        assert (fg == 0).all() if t < 20 else True
    eng.close()
    with pytest.raises(capi.BgsError):
        Engine(capi.VUMETER).set_eigen_params(history_size=4)


def test_host_class_through_frame_processor_round_trips_its_xml(tmp_path):
    """The C++ host layer: FrameProcessor with enableDPEigenbackgroundBGS, the h8_m3 case's values through
    ./config/DPEigenbackgroundBGS.xml, which must come back unchanged, in the reference's key order; masks equal the host path's."""
    from test_gpu_01_host_cpp import DEMO, HOST, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    r = en.load()["h8_m3"]
    n, rows, cols = r["masks"].shape
    name = "DPEigenbackgroundBGS"
    wd = tmp_path
    (wd / "config").mkdir(parents=True)
    raw = str(wd / "frames.raw")
    r["frames"].tofile(raw)
    p = r["params"]
    (wd / "config" / (name + ".xml")).write_text(
        '<?xml version="1.0"?>\n<opencv_storage>\n<threshold>%d</threshold>\n<historySize>%d</historySize>\n<embeddedDim>%d</embeddedDim>\n<showOutput>0</showOutput>\n</opencv_storage>\n'
        % (p["threshold"], p["history_size"], p["embedded_dim"]))
    write_fp_config(str(wd / "config"), set())
    path = str(wd / "config" / "FrameProcessor.xml")
    text = open(path).read().replace("</opencv_storage>", "<enable%s>1</enable%s>\n</opencv_storage>" % (name, name))
    open(path, "w").write(text)
    res = subprocess.run([DEMO, raw, str(rows), str(cols), str(n), str(wd / "out")], cwd=str(wd), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert name + "()" in res.stdout and "~" + name + "()" in res.stdout  # the reference's banners
    got = np.fromfile(str(wd / ("out.%s.raw" % name)), np.uint8).reshape(n, rows, cols)
    assert np.array_equal(got, single("h8_m3")[0]), int((got != single("h8_m3")[0]).sum())
    saved = (wd / "config" / (name + ".xml")).read_text()
    pos = [saved.index("<%s>" % k) for k in ("threshold", "historySize", "embeddedDim", "showOutput")]
    assert pos == sorted(pos) and "<historySize>8</historySize>" in saved and "<embeddedDim>3</embeddedDim>" in saved and "<showOutput>0</showOutput>" in saved, saved
