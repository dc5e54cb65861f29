"""The slot arithmetic of the frame history ring (tracking_amd/csrc/frame_history.h: the slot of the current frame, of its history, of
the planes prev1 / prev2, and the copies that bring the ring up to date after a clip call) against a naive simulation, under
AddressSanitizer and UBSan.  The checks are tests/frame_history_main.cpp, a program of its own: nothing of Python runs in the sanitized
process."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_frame_history_arithmetic_sanitized(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "the frame history test needs g++"
    exe = str(tmp_path / "frame_history")
    # -static-lib*: the sanitizer runtimes are linked into the program, which keeps them first in its link order without touching the
    # environment of the process
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HERE, "frame_history_main.cpp")], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith(", 0 checks failed"), r.stdout[-4000:]
