// kernel_t2f.h — package_bgs/tb type-2 fuzzy GMMs, one fused kernel:
//
//   dp_gmm_kernel<K, T2fModel<false>>  T2FGMM::SubtractPixel with TYPE_T2FGMM_UM  package_bgs/tb/T2FGMM.cpp:106-303  (T2FGMM_UM.cpp:29-83)
//   dp_gmm_kernel<K, T2fModel<true>>   T2FGMM::SubtractPixel with TYPE_T2FGMM_UV                                     (T2FGMM_UV.cpp:29-83)
//
// The source is dp/GrimsonGMM.cpp with another match distance (H per channel from |mu - pixel|, dist = HR^2 + HG^2 + HB^2) and a mean
// update that subtracts k * |d|: the mean only ever moves down.  The wrappers return the HIGH-threshold mask, Update() is empty and
// no background image is written.  Pixel bytes are taken in memory order.
// State: kernel_dp.h's tiled layout (256-pixel tiles, plane-major inside a tile, xcd_block) with FIVE float planes per mode
// {variance, muR, muG, muB, weight} and a count byte per pixel.  The struct's sixth field, `significants`, is never read before it is
// rewritten - both renormalisations assign it for every mode below the count before either sort - so it lives in registers only and
// bgs_get_state recomputes it (engine_t2f.h).  For the same reason the assignments to it inside the mode loop are not made here: the
// first renormalisation overwrites every one of them before anything reads them.
// So the kernel is kernel_dp.h's dp_gmm_kernel in its kDpT2f form (Grimson's steps, five planes per mode, the key in registers) with
// the model below plugged in: the kernel's argument type, the per-launch constants and the distance.
#pragma once
#include "kernel_dp.h"

namespace bgs {

struct T2fArgs {
  DpArgs d;      // frame / state / bstate (count bytes) / masks / clip strides: as for dp_gmm_kernel; low, high, alpha in the params' float
  float km, kv;  // T2FGMM::km / kv
};

template <bool UV>
struct T2fModel {
  using Args = T2fArgs;
  static constexpr DpGmm kSource = kDpT2f;
  // per-launch constants, each rounded where the source rounds it for every pixel
  float km, twoKm, halfKmKm;  // 2*km*d/var = ((2*km)*d)/var;  ... + km*km/2
  float uvFactor;             // (1/(kv*kv)-kv*kv)
  __device__ __forceinline__ explicit T2fModel(const Args& ta)
      : km(ta.km), twoKm(2 * ta.km), halfKmKm(ta.km * ta.km / 2), uvFactor(div_rn(1.0f, ta.kv * ta.kv) - ta.kv * ta.kv) {}
  __device__ __forceinline__ static const DpArgs& dp(const Args& ta) { return ta.d; }
  // dist = HR^2 + HG^2 + HB^2 with H per channel from d = |mu - pixel|; the mean update subtracts k * d
  __device__ __forceinline__ float distance(const float (&mu)[3], float var, const float (&px)[3], float (&d)[3]) const {
    float H[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      d[ch] = fabsf(mu[ch] - px[ch]);
      if constexpr (UV) {
        const float e = px[ch] - mu[ch];
        H[ch] = div_rn(uvFactor * e * e, 2 * var);
      } else {
        const float kmv = km * var;
        if (px[ch] < mu[ch] - kmv || px[ch] > mu[ch] + kmv)
          H[ch] = div_rn(twoKm * d[ch], var);
        else
          H[ch] = div_rn(d[ch] * d[ch], 2 * var * var) + div_rn(km * d[ch], var) + halfKmKm;
      }
    }
    return (H[0] * H[0] + H[1] * H[1] + H[2] * H[2]);
  }
};

}  // namespace bgs
