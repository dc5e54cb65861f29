"""kernel_mog2.h, mog2_smin: the filter kernel's rejection rule as ONE compare.  The rule was S > 3 && (8 S - 28)^2 > tq in 32-bit
unsigned arithmetic, per summary; it is monotone in the bucket distance S, so the host now hands the kernel s_min, the smallest S
that passes.  A stand-alone host program (its own main, no GPU call) includes the kernel header and compares the two predicates for
every S the three 5-bit buckets can produce (0 .. 93) at every tq where the answer can flip, plus the ends."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include "kernel_mog2.h"
#include <cstdio>
#include <vector>
using namespace bgs;
static bool old_rule(uint32_t word, uint32_t S, uint32_t tq) {
  const uint32_t B = 8u * S - 28u;  // wraps for S < 4: caught by the first test
  return S > 3u && !(word >> 15) && B * B > tq;
}
int main() {
  std::vector<uint32_t> tqs = {0u, 1u, 3u, 4u, 15u, 16u, 17u, 0xfffffffeu, 0xffffffffu /* the clamp */, mog2_tq(0.f), mog2_tq(1e-3f),
                               mog2_tq(9.f), mog2_tq(16.f), mog2_tq(4e3f), mog2_tq(1e9f), mog2_tq(-1.f)};
  for (uint32_t S = 4; S <= 93; ++S) {
    const uint32_t B = 8u * S - 28u, q = B * B;
    tqs.push_back(q - 1u), tqs.push_back(q), tqs.push_back(q + 1u);
  }
  if (kMog2SMax != 93u) return std::printf("kMog2SMax %u\n", kMog2SMax), 1;
  long checked = 0, bad = 0;
  for (uint32_t tq : tqs) {
    const uint32_t s_min = mog2_smin(tq);
    for (uint32_t S = 0; S <= 93; ++S)
      for (uint32_t word : {0u, 0x7fffu, 0x8000u, 0xffffu}) {  // class 0 / class 1, whatever the buckets
        ++checked;
        if (mog2_reject_s(word, S, s_min) != old_rule(word, S, tq)) {
          if (++bad < 10) std::printf("tq %u s_min %u S %u word %#x: new %d old %d\n", tq, s_min, S, word, (int)mog2_reject_s(word, S, s_min), (int)old_rule(word, S, tq));
        }
      }
  }
  // the spread puts the three buckets into the bytes the pixel's own buckets (mog2_pixq) occupy
  for (uint32_t w = 0; w < 0x10000u; ++w) {
    const uint32_t want = (w & 0x1fu) | (((w >> 5) & 0x1fu) << 8) | (((w >> 10) & 0x1fu) << 16);
    ++checked;
    if (mog2_spread(w) != want && ++bad < 10) std::printf("spread %#x: %#x, want %#x\n", w, mog2_spread(w), want);
  }
  if (mog2_smin(0xffffffffu) != kMog2SNever || mog2_smin(mog2_tq(1e9f)) != kMog2SNever) return std::printf("the clamp must reject nothing\n"), 1;
  if (mog2_smin(0u) != 4u) return std::printf("s_min(0) = %u\n", mog2_smin(0u)), 1;
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
"""


def test_smin_rule_equals_the_squared_rule(tmp_path):
    src = tmp_path / "smin_check.hip"
    exe = tmp_path / "smin_check"
    src.write_text(PROGRAM)
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "tracking_amd", "csrc"), "-o", str(exe), str(src)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    n = 94 * 4 * (16 + 3 * 90) + 0x10000
    assert run.stdout.strip().endswith("checked %d bad 0" % n), run.stdout[-500:]
