"""Writes tests/golden/dp_ref_{ziv,grim,wren,mean,median}.npz from oracle/_ref/ref_dp_cli: the reference's own package_bgs/dp
model files compiled unmodified (oracle/Makefile) and driven in the DP*BGS wrappers' order (oracle/ref_dp_cli.cpp).  Needs the
reference tree at build time, so it runs where `make -C oracle` built oracle/_ref; the tests need only the files it wrote.

    python tests/golden/make_dp_ref.py [--check]     --check: write nothing, fail if a file on disk would change

Every case (tests/dp_ref.py: cases) runs twice, each time in a fresh process, with two different bytes in every image buffer the
reference allocates (REF_STUB_POISON): the two outputs must agree byte for byte, otherwise the reference read memory it never
wrote and the case is not written.  The DPGrimsonGMM cases also run on the build whose unqualified sqrt() is the double
overload; the cases on which that changes any bit are recorded in `environment`, next to the overload of the pinned build.
The output is deterministic: seeded inputs, one thread, and an archive written with fixed timestamps (tests/dp_ref.py: save)."""
import json
import os
import platform
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, os.pardir, os.pardir), os.path.join(HERE, os.pardir)]

import dp_ref  # noqa: E402
from oracle import pyoracle  # noqa: E402

POISON = (0xCD, 0x11)


def main():
    check = "--check" in sys.argv[1:]
    assert pyoracle.ref_dp_available(), "oracle/_ref/ref_dp_cli is missing: run `make -C oracle` where the reference tree is present"
    exe = os.path.join(os.path.dirname(pyoracle._REF_DP), "ref_dp_cli")
    overload = subprocess.run([exe, "env"], capture_output=True, text=True, check=True).stdout.strip()
    status = 0
    for cls in dp_ref.CLASSES:
        arrays, names, sqrt_double_differs = {}, [], []
        for case, p in dp_ref.cases(cls).items():
            frames = dp_ref.frames_of(p)
            T, H, W = frames.shape[:3]
            kw = dp_ref.ref_kwargs(cls, p)
            runs = [pyoracle.ref_dp_clip(cls, frames, planes=True, poison=b, **kw) for b in POISON]
            (masks, model), (masks2, model2) = runs
            if not (np.array_equal(masks, masks2) and all(dp_ref.same_bits(model[k], model2[k]) for k in model)):
                print("%s/%s: the two poison runs differ - the reference reads uninitialised memory; case NOT written" % (cls, case))
                status = 1
                continue
            if cls == "grim":
                m3, model3 = pyoracle.ref_dp_clip(cls, frames, planes=True, exe=exe + "_sqrtd", **kw)
                if not (np.array_equal(masks, m3) and all(dp_ref.same_bits(model[k], model3[k]) for k in model)):
                    sqrt_double_differs.append(case)
            names.append(case)
            arrays[case + "/params"] = np.array(json.dumps(p, sort_keys=True))
            arrays[case + "/input_crc32"] = np.array(dp_ref.crc(frames), np.uint32)
            arrays[case + "/shape"] = np.array([T, H, W], np.int32)
            arrays[case + "/masks"] = np.packbits(masks.reshape(T, H, W) != 0, axis=-1)
            if H * W <= dp_ref.PLANE_PIXELS * 1.05:
                for k, v in model.items():
                    arrays[case + "/" + k] = v.view(np.uint32) if v.dtype == np.float32 else v
        env = {"sqrt_overload": overload, "sqrt_double_changes_cases": sqrt_double_differs, "poison_bytes": list(POISON),
               "flags": "g++ -O2 -ffp-contract=off -std=gnu++0x", "libc": " ".join(platform.libc_ver())}
        arrays["cases"] = np.array(json.dumps(names))
        arrays["environment"] = np.array(json.dumps(env, sort_keys=True))
        path = os.path.join(HERE, "dp_ref_%s.npz" % cls)
        tmp = path + ".tmp"
        dp_ref.save(tmp, arrays)
        new = open(tmp, "rb").read()
        same = os.path.exists(path) and open(path, "rb").read() == new
        print("%-6s %2d cases %6d bytes %s  sqrt-double changes: %s" % (cls, len(names), len(new), "unchanged" if same else "CHANGED", sqrt_double_differs or "none"))
        assert len(new) <= 128 * 1024, "fixture larger than 128 KB"
        if check:
            os.remove(tmp)
            status |= not same
        else:
            os.replace(tmp, path)
    return status


if __name__ == "__main__":
    sys.exit(main())
