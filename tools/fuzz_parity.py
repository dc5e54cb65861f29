"""Randomised differential test of the HIP path (GPU box): random class, geometry (odd sizes included), parameters inside the ranges
the engine accepts, number of streams, and a random mix of entry points (host frames, device batches, device ranges, clips).  Every
mask, every background the class delivers and - where the helpers know the model - the state at the end must match.

Two tables.  The default one (`ALL`) holds the classes oracle/bgs_oracle.c restates and compares the engine with that oracle.
`models` holds the 16 classes that are pinned to reference-built fixtures (KDE, DPPratiMediod, DPTexture, the five lb/ models, VuMeter,
the fuzzy integrals, T2FGMM_UM / _UV, DPEigenbackground, IndependentMultimodalBGS, MultiLayerBGS) and compares the engine with their numpy restatements through the adapters of
tests/model_refs.py, each under its class's written contract.

A case is drawn without a GPU - draw_case(rng, seed, table) returns its description - and then run: run_case(case).

Usage: python tools/fuzz_parity.py [seconds] [seed] [models] [big] [v]; prints one line per case, exits 1 on the first mismatch with
the seed that reproduces it, and ends with the cases per class, the rejected ones and the mismatches.  "big" = frames of several tiles
(33x64 .. 200x320; a family whose restatement is slow keeps its own, smaller list), "v" = print each case before it runs; after `models`,
class or family names (`models imbs big`) keep the run to those."""
import sys
import time

import numpy as np

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
from gpu_helpers import ALGOS, check_state, check_subsense_state  # noqa: E402
from oracle import pyoracle  # noqa: E402
from tracking_amd import Engine, capi  # noqa: E402

VERBOSE = False
BIG = False
ALL = dict(ALGOS)
ALL["SuBSENSEBGS"] = capi.SUBSENSE
ALL["LOBSTERBGS"] = capi.LOBSTER


def rand_params(rng, name):
    kw = {}
    if rng.random() < 0.3:
        kw["threshold"] = int(rng.integers(0, 60))
    if rng.random() < 0.15 and name not in ("SuBSENSEBGS", "LOBSTERBGS", "GMG"):
        kw["enable_threshold"] = 0
    if name in ("MixtureOfGaussianV2BGS", "MixtureOfGaussianV1BGS", "AdaptiveBackgroundLearning"):
        kw["alpha"] = float(rng.choice([-1.0, 0.001, 0.01, 0.05, 0.2, 0.7])) if name != "AdaptiveBackgroundLearning" else float(rng.choice([0.01, 0.05, 0.3]))
    if name == "MixtureOfGaussianV2BGS":
        if rng.random() < 0.5:
            kw.update(mog2_var_threshold=float(rng.choice([4, 16, 36])), mog2_background_ratio=float(rng.choice([0.5, 0.9])), mog2_ct=float(rng.choice([0.0, 0.05, 0.3])),
                      mog2_history=int(rng.choice([3, 20, 500])), mog2_detect_shadows=int(rng.integers(0, 2)))
    if name == "MixtureOfGaussianV1BGS" and rng.random() < 0.5:
        kw.update(mog1_history=int(rng.choice([2, 10, 200])), mog1_background_ratio=float(rng.choice([0.4, 0.7, 0.95])), mog1_noise_sigma=float(rng.choice([5.0, 15.0])))
    if name in ("WeightedMovingMeanBGS", "WeightedMovingVarianceBGS"):
        kw["enable_weight"] = int(rng.integers(0, 2))
    if name == "AdaptiveSelectiveBackgroundLearning":
        kw.update(learning_frames=int(rng.choice([2, 5, 90])), alpha_learn=float(rng.choice([0.05, 0.3])), alpha_detection=float(rng.choice([0.05, 0.2])))
    if name == "SigmaDeltaBGS":
        kw.update(sd_amp_factor=int(rng.choice([1, 2, 4, 300])), sd_min_var=int(rng.choice([1, 15])), sd_max_var=int(rng.choice([100, 255])))
    if name.startswith("DP"):
        kw.update(dp_threshold=float(rng.choice([9.0, 16.0, 40.0])), dp_alpha=float(rng.choice([1e-4, 0.01, 0.3])), dp_gaussians=int(rng.integers(1, 6)),
                  dp_sampling_rate=int(rng.choice([2, 7])), learning_frames=int(rng.choice([3, 30])))
    if name in ("SuBSENSEBGS", "LOBSTERBGS"):
        ns = int(rng.choice([3, 7, 20, 35, 50]))
        kw.update(subsense_n_samples=ns, subsense_n_required=int(rng.integers(1, min(ns, 3) + 1)), lbsp_rel_threshold=float(rng.choice([0.2, 0.333, 0.365])),
                  subsense_min_color_dist_threshold=int(rng.choice([15, 30])), subsense_desc_dist_threshold_offset=int(rng.choice([1, 3, 4])))
    if name == "GMG":
        kw.update(gmg_init_frames=int(rng.choice([3, 8])), gmg_max_features=int(rng.choice([8, 64])), gmg_smoothing_radius=int(rng.choice([3, 7])))
    return kw


def draw_frames(rng, seed):
    """The recipe of one stream's clip; frames_of() makes the frames."""
    kind = str(rng.choice(["random", "surv", "smooth", "sat"]))
    return dict(kind=kind, seed=seed, cut=bool(rng.random() < 0.3))  # cut: a scene cut half-way


def frames_of(recipe, T, H, W):
    from tools import synth
    if recipe["kind"] == "random":
        f = synth.random_frames(T, H, W, 3, seed=recipe["seed"])
    else:
        f = synth.numpy_frames(recipe["kind"], T, H, W, seed=recipe["seed"])
    if recipe["cut"]:
        c = T // 2
        f = np.concatenate([f[:c], 255 - f[c:]])
    return np.ascontiguousarray(f)


def draw_case(rng, seed, table="all", big=None):
    """The description of case `seed`: class, H, W, S, T, parameters, input recipes, entry-point schedule, reset schedule (and, for
    the models, the parameter switch).  Pure: no torch, no engine, and for the default table the order of the rng calls of every
    earlier version of this tool, so a seed keeps meaning the case it always meant.  table: "all", "models", a family of
    tests/model_refs.py, or a list of its class names."""
    big = BIG if big is None else big
    if table != "all":
        import model_refs
        classes = model_refs.MODELS if table == "models" else model_refs.FAMILIES[table] if isinstance(table, str) else list(table)
        return model_refs.draw_model_case(rng, seed, classes, big)
    name = str(rng.choice(sorted(ALL)))
    small = name in ("SuBSENSEBGS", "LOBSTERBGS", "GMG")
    if big:  # several tiles in both directions, ragged edges
        H, W = int(rng.choice([33, 65, 97, 130, 200])), int(rng.choice([64, 97, 131, 257, 320]))
    else:
        H = int(rng.choice([5, 9, 16, 33, 48] if small else [1, 7, 16, 33, 64]))
        W = int(rng.choice([5, 37, 64, 131] if small else [3, 64, 70, 128, 200]))
    S = int(rng.integers(1, 4))
    T = int(rng.integers(4, 22))
    kw = rand_params(rng, name)
    inputs = [draw_frames(rng, seed * 7 + s) for s in range(S)]
    mode = str(rng.choice(["host", "batch", "clip", "mixed"]))
    if name == "MixtureOfGaussianV2BGS":  # round 3: which MOG2 kernel loads the model (dense / eager / count / auto / filter)
        kw["sparse"] = int(rng.choice([0, 1, 2, 3, 4]))
    resets = bool(rng.random() < 0.35)  # round 3: cameras of a batch are reset independently, so the streams of one call have different ages
    steps, t = [], 0
    while t < T:
        st = dict(t=t, n=1, resets=[])
        if resets and t > 0 and rng.random() < 0.3:
            st["resets"].append(int(rng.integers(0, S)))
        st["m"] = mode if mode != "mixed" else str(rng.choice(["host", "batch", "clip"]))
        if st["m"] == "clip":
            st["n"] = int(min(T - t, rng.integers(1, 12)))
        steps.append(st)
        t += st["n"]
    return dict(table="all", seed=int(seed), big=bool(big), name=name, H=H, W=W, S=S, T=T, params=kw, inputs=inputs, mode=mode, resets=resets, steps=steps)


def run_case(case):
    """Run a drawn case on the GPU; returns its one-line result, raises AssertionError on a mismatch."""
    if case["table"] == "models":
        return run_model_case(case)
    import torch
    name, H, W, S, T, mode, resets = (case[k] for k in ("name", "H", "W", "S", "T", "mode", "resets"))
    algo = ALL[name]
    kw = dict(case["params"])
    level = kw.pop("sparse", None)
    p = capi.default_params(algo)
    for k, v in kw.items():
        setattr(p, k, v)
    clips = np.stack([frames_of(r, T, H, W) for r in case["inputs"]])  # [S][T][H][W][3]
    if VERBOSE:
        print("case %d: %s %dx%d x%d streams, %d frames, %s" % (case["seed"], name, W, H, S, T, kw), flush=True)
    want_bits = (H * W) % 64 == 0
    try:
        eng = Engine(algo, params=p, n_streams=S)
        orcs = [pyoracle.Oracle(algo, params=p) for _ in range(S)]
    except capi.BgsError as e:
        return "%s rejected %s: %s" % (name, kw, e)
    try:
        eng.set_geometry(H, W, 3)
    except capi.BgsError as e:
        eng.close()
        return "%s %dx%d not supported: %s" % (name, W, H, str(e)[:60])
    if level is not None:
        eng.set_option(capi.OPT_MOG2_SPARSE, level)
        kw["sparse"] = level
    for st in case["steps"]:
        t, n, m = st["t"], st["n"], st["m"]
        for r in st["resets"]:
            eng.reset_stream(r)
            orcs[r].close()
            orcs[r] = pyoracle.Oracle(algo, params=p)
        if m == "host":
            got = []
            for s in range(S):
                fg, bg = eng.process(clips[s, t], stream=s)
                got.append((fg, bg))
            outs = [[g] for g in got]
        else:
            d = torch.from_numpy(np.ascontiguousarray(clips[:, t:t + n].transpose(1, 0, 2, 3, 4))).cuda()
            fg = torch.full((n, S, H, W), 7, dtype=torch.uint8, device="cuda")
            bits = torch.zeros((n, S, H * W // 64), dtype=torch.int64, device="cuda") if want_bits else None
            if m == "batch":
                eng.process_batch_device(d[0], fg[0], None, bits[0] if want_bits else None)
            else:
                eng.process_clip_device(d, n, fg, None, bits)
            torch.cuda.synchronize()
            fgh = fg.cpu().numpy()
            outs = [[(fgh[j, s], None) for j in range(n)] for s in range(S)]  # validity per stream: an untouched output keeps the marker 7
            if want_bits:
                bh = np.unpackbits(bits.cpu().numpy().view(np.uint8).reshape(n, S, -1), axis=2, bitorder="little").reshape(n, S, H, W)
        for s in range(S):
            for j in range(n):
                ofg, obg = orcs[s].process(clips[s, t + j])
                fg_j, bg_j = outs[s][j]
                if m == "host":
                    assert (fg_j is None) == (ofg is None), "%s frame %d stream %d: mask validity" % (name, t + j, s)
                elif ofg is None:
                    assert (fg_j == 7).all(), "%s frame %d stream %d (%s): a warm-up frame must leave the mask untouched" % (name, t + j, s, m)
                if ofg is not None:
                    assert np.array_equal(fg_j, ofg), "%s frame %d stream %d (%s): %d mask pixels differ" % (name, t + j, s, m, int((fg_j != ofg).sum()))
                    if m != "host" and want_bits:
                        assert np.array_equal(bh[j, s] * 255, np.where(ofg != 0, 255, 0)), "%s frame %d stream %d: packed mask" % (name, t + j, s)
                if m == "host":
                    assert (bg_j is None) == (obg is None), "%s frame %d: background validity" % (name, t + j)
                    if obg is not None:
                        assert np.array_equal(bg_j.reshape(obg.shape), obg), "%s frame %d stream %d: background differs" % (name, t + j, s)
    for s in range(S):
        if name == "SuBSENSEBGS":
            check_subsense_state(eng, orcs[s], H, W, nS=p.subsense_n_samples, stream=s)
        elif name.startswith("DP"):
            from gpu_helpers import check_dp_state
            check_dp_state(name, eng, orcs[s], H * W, K=p.dp_gaussians, stream=s)
        elif name == "GMG":
            F, n = p.gmg_max_features, H * W
            assert np.array_equal(eng.get_state("nfeatures", (n,), np.int32, stream=s), orcs[s].get_state("nfeatures", (n,), np.int32)), "GMG feature counts"
            assert np.array_equal(eng.get_state("colors", (F, n), np.int32, stream=s), orcs[s].get_state("colors", (F, n), np.int32)), "GMG colours"
            assert float(np.max(np.abs(eng.get_state("weights", (F, n), np.float32, stream=s) - orcs[s].get_state("weights", (F, n), np.float32)))) <= 1e-4, "GMG weights"
        else:
            check_state(name, eng, orcs[s], H * W, stream=s)
    eng.close()
    return "%s %dx%d x%d streams, %d frames, %s%s %s: ok" % (name, W, H, S, T, mode, " +resets" if resets else "", kw)


def run_model_case(case):
    """A case of the `models` table: the engine through the case's entry points against reference_run's restatement."""
    import model_refs as mr
    import torch
    name, H, W, S = case["name"], case["H"], case["W"], case["S"]
    ad = mr.BY_CLASS[name]
    if VERBOSE:
        print("case %d: %s" % (case["seed"], mr.describe(case)), flush=True)
    must_refuse = ad.refusal(name, case["params"])
    try:
        eng = ad.make_engine(name, case["params"], S)
    except capi.BgsError as e:  # construction / set_params: before a device is opened
        assert must_refuse is not None, "%s refused parameters its contract accepts, %s: %s" % (name, case["params"], e)
        assert e.code == must_refuse and ad.needle(name) in str(e), "%s: refusal %d '%s' must carry code %d and name the class" % (name, e.code, e, must_refuse)
        return "%s rejected %s: %s" % (name, case["params"], e)
    try:
        assert must_refuse is None, "%s accepted %s, which its contract refuses (%s)" % (name, case["params"], case["bad"])
        eng.set_geometry(H, W, 3)
        frames = mr.build_inputs(case)
        outs, refs, _ = mr.reference_run(case, frames)
        _drive(torch, mr, ad, eng, case, frames, outs)
        cur = _in_force(ad, case)
        for s in range(S):
            want = ad.normalise(name, refs[s].planes())
            got = ad.normalise(name, {k: eng.get_state(k, np.shape(v), ad.fetch.get(k, np.asarray(v).dtype), stream=s) for k, v in want.items()})
            mr.check_planes(got, want, ad.tols.get(name, {}), "%s stream %d at the end (%s)" % (name, s, cur))
    finally:
        eng.close()
    return "%s: ok" % mr.describe(case)


def _in_force(ad, case):
    sw = case["switch"]
    return ad.follow(case["name"], case["params"], sw["params"]) if sw else case["params"]


def _drive(torch, mr, ad, eng, case, frames, outs):
    name, H, W, S = case["name"], case["H"], case["W"], case["S"]
    Wd = (H * W + 63) // 64
    bgs = ad.bg_shape(H, W) if ad.has_bg else None
    sw = case["switch"]
    side = None
    for st in case["steps"]:
        t, n, m = st["t"], st["n"], st["m"]
        if sw and t == sw["t"]:
            ad.apply(eng, name, sw["params"])
        for r in st["resets"]:
            eng.reset_stream(r)
        got = [[None] * n for _ in range(S)]  # (mask or None, background or None, packed words or None)
        if m == "host":
            for s in range(S):
                fg, bg = eng.process(frames[s, t], stream=s, want_bg=ad.has_bg)
                got[s][0] = (fg, bg, None)
        elif m == "submit":
            fgs = [np.full((H, W), mr.FG_MARK, np.uint8) for _ in range(S)]
            bgh = [np.full(bgs, mr.BG_MARK, np.uint8) if bgs else None for _ in range(S)]
            for s in range(S):
                eng.submit(frames[s, t], fgs[s], bgh[s], stream=s)
            for s in range(S):
                fl = eng.wait(stream=s)
                if not fl & capi.FG_VALID:
                    assert (fgs[s] == mr.FG_MARK).all(), "%s frame %d stream %d (submit): a frame without a mask must leave the buffer untouched" % (name, t, s)
                if bgs and not fl & capi.BG_VALID:
                    assert (bgh[s] == mr.BG_MARK).all(), "%s frame %d stream %d (submit): a frame without a background must leave the buffer untouched" % (name, t, s)
                got[s][0] = (fgs[s] if fl & capi.FG_VALID else None, bgh[s] if bgs and fl & capi.BG_VALID else None, None)
        else:
            d = torch.from_numpy(np.ascontiguousarray(frames[:, t:t + n].transpose(1, 0, 2, 3, 4))).cuda()
            fg = torch.full((n, S, H, W), mr.FG_MARK, dtype=torch.uint8, device="cuda")
            bg = torch.full((n, S) + bgs, mr.BG_MARK, dtype=torch.uint8, device="cuda") if bgs else None
            bits = torch.full((n, S, Wd), -1, dtype=torch.int64, device="cuda")
            if m == "batch":
                eng.process_batch_device(d[0], fg[0], bg[0] if bgs else None, bits[0])
            elif m == "clip":
                eng.process_clip_device(d, n, fg, bg, bits)
            else:  # two stream ranges on two HIP streams, each ordered after the upload
                if side is None:
                    side = (torch.cuda.Stream(), torch.cuda.Stream())
                torch.cuda.current_stream().synchronize()
                k = st["split"]
                for q, (a, b) in zip(side, ((0, k), (k, S))):
                    if b > a:
                        eng.process_batch_device(d[0, a:b], fg[0, a:b], bg[0, a:b] if bgs else None, bits[0, a:b], hip_stream=q.cuda_stream, first=a, count=b - a)
                for q in side:
                    q.synchronize()
            torch.cuda.synchronize()
            fgh, bgh, bh = fg.cpu().numpy(), bg.cpu().numpy() if bgs else None, bits.cpu().numpy().view(np.uint64)
            for s in range(S):
                for j in range(n):
                    got[s][j] = (fgh[j, s], bgh[j, s] if bgs else None, bh[j, s])
        for s in range(S):
            for j in range(n):
                wfg, wbg, ignore = outs[s][t + j]
                fg_j, bg_j, bits_j = got[s][j]
                where = "%s frame %d stream %d (%s)" % (name, t + j, s, m)
                if m in ("host", "submit"):
                    assert (fg_j is None) == (wfg is None), where + ": mask validity"
                    assert (bg_j is None) == (wbg is None), where + ": background validity"
                else:
                    if wfg is None:
                        assert (fg_j == mr.FG_MARK).all(), where + ": a frame without a mask must leave the buffer untouched"
                    if bgs and wbg is None:
                        assert (bg_j == mr.BG_MARK).all(), where + ": a frame without a background must leave the buffer untouched"
                if wfg is not None:
                    mr.check_mask(fg_j, wfg, where, ignore)
                    if bits_j is not None:
                        assert np.array_equal(bits_j, mr.words_of(fg_j)), where + ": packed words differ from the byte mask (tail bits must be zero)"
                if wbg is not None:
                    mr.check_background(bg_j, wbg, where)


def one_case(rng, case_seed):
    """A case of the default table, drawn and run (tests/test_gpu_08_fuzz.py)."""
    return run_case(draw_case(rng, case_seed, "all"))


def main():
    global VERBOSE, BIG
    VERBOSE = "v" in sys.argv[3:]
    BIG = "big" in sys.argv[3:]
    table, words = "all", ""
    if "models" in sys.argv[3:]:
        import model_refs
        picked = [w for w in sys.argv[3:] if w in model_refs.MODELS or w in model_refs.FAMILIES]  # `models KDE lb`: these classes / families only
        table = sorted({c for w in picked for c in model_refs.FAMILIES.get(w, [w])}) or "models"
        words = " models" + "".join(" " + w for w in picked)
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else int(time.time()) % 100000
    t0 = time.time()
    k = 0
    ran, rejected = {}, {}
    failed = None
    while time.time() - t0 < budget:
        case_seed = seed0 + k
        case = draw_case(np.random.default_rng(case_seed), case_seed, table)
        sys.stderr.write("seed %d\n" % case_seed)  # unbuffered: a case that ends the process has named itself
        try:
            msg = run_case(case)
        except AssertionError as e:
            print("MISMATCH (seed %d): %s" % (case_seed, e), flush=True)
            print("reproduce: python tools/fuzz_parity.py 0.001 %d%s%s v" % (case_seed, words, " big" if BIG else ""), flush=True)
            failed = case_seed
            break
        print("[%d] %s" % (case_seed, msg), flush=True)
        tally = ran if msg.endswith(": ok") else rejected
        tally[case["name"]] = tally.get(case["name"], 0) + 1
        k += 1
    print("table %s%s, seeds %d..%d, %.0f s" % (words.strip() or "all", " big" if BIG else "", seed0, seed0 + max(k - 1, 0), time.time() - t0))
    for name in sorted(set(ran) | set(rejected)):
        print("  %-28s %5d ok %4d rejected" % (name, ran.get(name, 0), rejected.get(name, 0)))
    print("%d cases, %d rejected, %d mismatches" % (k, sum(rejected.values()), 0 if failed is None else 1))
    if failed is not None:
        sys.exit(1)
    print("%d cases in %.0f s, no mismatch" % (k, time.time() - t0))


if __name__ == "__main__":
    main()
