"""Fixed slices of the randomised differential run of the 16 reference-pinned model classes (tools/fuzz_parity.py `models`) inside the
GPU suite: KDE, DPPratiMediod, DPTexture, the five lb/ models, VuMeter, the fuzzy integrals, T2FGMM_UM / _UV, DPEigenbackground,
IndependentMultimodalBGS and MultiLayerBGS against their numpy restatements, through random geometries (one-row, narrow, ragged, several tiles), parameters (one the engine must
refuse among them), 1-3 streams, every entry point (host frames, submit / wait, device batches, two ranges on two HIP streams, clips of
1-11 frames, a mix), independent stream resets and parameter switches.  Masks, backgrounds, packed words and the model at the end,
each under its class's written contract (tests/model_refs.py).  tests/test_fuzz_models_cpu.py holds the slices to what a class needs.

Seeds are fixed.  A case writes its seed to stderr before it runs, so one that ends the process has named itself; a failing case
prints the command that reproduces it."""
import os

import numpy as np
import pytest

import model_refs as mr

pytestmark = pytest.mark.gpu


def run_seed(seed, classes, big, capfd):
    from tools import fuzz_parity
    with capfd.disabled():  # the real stderr, not pytest's capture file, and unbuffered
        os.write(2, ("fuzz models %s%s: seed %d\n" % (" ".join(classes), " big" if big else "", seed)).encode())
    case = fuzz_parity.draw_case(np.random.default_rng(seed), seed, list(classes), big=big)
    from tracking_amd import capi
    try:
        return fuzz_parity.run_case(case)
    except capi.BgsError as e:
        if e.code == capi.ERR_HIP:  # the device reported an error: nothing more is started on it from this process
            pytest.exit("seed %d (models %s%s): %s" % (seed, " ".join(classes), " big" if big else "", e), returncode=3)
        raise
    except AssertionError as e:
        raise AssertionError("%s\nreproduce: python tools/fuzz_parity.py 0.001 %d models %s%s v" % (e, seed, " ".join(classes), " big" if big else "")) from None


@pytest.mark.parametrize("classes,big,first,count", [s[1:] for s in mr.SLICES], ids=[s[0] for s in mr.SLICES])
def test_fixed_slice_of_the_models_fuzz(classes, big, first, count, capfd):
    ran = sum(run_seed(seed, classes, big, capfd).endswith(": ok") for seed in range(first, first + count))
    assert ran >= count // 2, "most cases must be accepted by the engine (%d of %d ran)" % (ran, count)
