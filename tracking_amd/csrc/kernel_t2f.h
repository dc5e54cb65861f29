// kernel_t2f.h — package_bgs/tb type-2 fuzzy GMMs, one fused kernel:
//
//   t2f_gmm_kernel<K, false>  T2FGMM::SubtractPixel with TYPE_T2FGMM_UM  package_bgs/tb/T2FGMM.cpp:106-303  (T2FGMM_UM.cpp:29-83)
//   t2f_gmm_kernel<K, true>   T2FGMM::SubtractPixel with TYPE_T2FGMM_UV                                     (T2FGMM_UV.cpp:29-83)
//
// The source is dp/GrimsonGMM.cpp with another match distance (H per channel from |mu - pixel|, dist = HR^2 + HG^2 + HB^2) and a mean
// update that subtracts k * |d|: the mean only ever moves down.  The wrappers return the HIGH-threshold mask, Update() is empty and
// no background image is written.  Pixel bytes are taken in memory order.
// State: kernel_dp.h's tiled layout (256-pixel tiles, plane-major inside a tile, xcd_block) with FIVE float planes per mode
// {variance, muR, muG, muB, weight} and a count byte per pixel.  The struct's sixth field, `significants`, is never read before it is
// rewritten - both renormalisations assign it for every mode below the count before either sort - so it lives in registers only and
// bgs_get_state recomputes it (engine_t2f.h).  For the same reason the assignments to it inside the mode loop are not made here: the
// first renormalisation overwrites every one of them before anything reads them.
// Control flow as in the source, statement by statement, with all indices static after unrolling (see dp_gmm_kernel).
#pragma once
#include "kernel_dp.h"

namespace bgs {

struct T2fArgs {
  DpArgs d;      // frame / state / bstate (count bytes) / masks / clip strides: as for dp_gmm_kernel; low, high, alpha in the params' float
  float km, kv;  // T2FGMM::km / kv
};

template <int K, bool UV>
__global__ __launch_bounds__(kBlock) void t2f_gmm_kernel(const T2fArgs ta) {
  constexpr int F = 5;
  constexpr int VAR = 0, MU = 1, WEIGHT = 4;
  const DpArgs& a = ta.d;
  const size_t gp = xcd_block(a.xcd_swizzle) * kBlock + threadIdx.x;
  const bool active = gp < a.npix;
  const int T = a.frames > 0 ? a.frames : 1;  // clip launches: the model stays in registers in between
  float* st = nullptr;
  uint8_t* pn = nullptr;
  int nModes = 0, nLoaded = 0, nUsed = 0;
  float g[K][F], sig[K];
  uint32_t g0[K][F];
  uint32_t pw = 0;
  if (active) {
    st = dp_plane0(a, gp, K * F);
    pn = a.bstate + (size_t)a.first * a.n + gp;
    pw = (uint32_t)a.frame[gp * 3] | ((uint32_t)a.frame[gp * 3 + 1] << 8) | ((uint32_t)a.frame[gp * 3 + 2] << 16);
    // Data-dependent traffic (exact), as in dp_gmm_kernel: the source never reads a mode at an index >= the pixel's count, so only
    // the used modes are loaded; at the end a field is stored if its bits changed, or unconditionally when its slot came into use.
    nModes = *pn;
    nLoaded = nModes;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      sig[k] = 0.f;
#pragma unroll
      for (int f = 0; f < F; ++f) {
        g[k][f] = k < nLoaded ? st[(k * F + f) * kDpTile] : 0.f;
        g0[k][f] = __float_as_uint(g[k][f]);
      }
    }
  }
  // per-launch constants, each rounded where the source rounds it for every pixel
  const float km = ta.km, kv = ta.kv;
  const float twoKm = 2 * km, halfKmKm = km * km / 2;        // 2*km*d/var = ((2*km)*d)/var;  ... + km*km/2
  const float uvFactor = div_rn(1.0f, kv * kv) - kv * kv;    // (1/(kv*kv)-kv*kv)
  for (int t = 0; t < T; ++t) {
    int mask = 0;
    if (active) {
      const float px[3] = {(float)(pw & 0xffu), (float)((pw >> 8) & 0xffu), (float)(pw >> 16)};
      if (t + 1 < T) {  // the next frame's pixel, requested before this frame's arithmetic
        const uint8_t* nf = a.frame + (size_t)(t + 1) * a.frame_stride + gp * 3;
        pw = (uint32_t)nf[0] | ((uint32_t)nf[1] << 8) | ((uint32_t)nf[2] << 16);
      }
      const float m_bg_threshold = 0.75f, m_variance = 36.0f;
      const float Alpha = a.alpha;
      bool bFitsPDF = false, bBackgroundHigh = false;
      const float fOneMinAlpha = 1 - Alpha;
      float totalWeight = 0.0f;
      int backgroundGaussians = 0;
      {
        double sum = 0.0;
        bool stop = false;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (k < nModes && !stop) {
            if (sum < (double)m_bg_threshold) {
              backgroundGaussians++;
              sum = __dadd_rn(sum, (double)g[k][WEIGHT]);
            } else
              stop = true;
          }
      }
      auto swap_modes = [&](int x, int y) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
          const float tmp = g[x][f];
          g[x][f] = g[y][f], g[y][f] = tmp;
        }
        const float ts = sig[x];
        sig[x] = sig[y], sig[y] = ts;
      };
#pragma unroll
      for (int im = 0; im < K; ++im) {
        if (im < nModes) {  // nModes may shrink inside the loop, as in the source
          float weight = g[im][WEIGHT];
          bool matched = false;
          if (!bFitsPDF) {
            const float var = g[im][VAR];
            float H[3], d[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const float mu = g[im][MU + ch];
              d[ch] = fabsf(mu - px[ch]);
              if constexpr (UV) {
                const float e = px[ch] - mu;
                H[ch] = div_rn(uvFactor * e * e, 2 * var);
              } else {
                const float kmv = km * var;
                if (px[ch] < mu - kmv || px[ch] > mu + kmv)
                  H[ch] = div_rn(twoKm * d[ch], var);
                else
                  H[ch] = div_rn(d[ch] * d[ch], 2 * var * var) + div_rn(km * d[ch], var) + halfKmKm;
              }
            }
            const float dist = (H[0] * H[0] + H[1] * H[1] + H[2] * H[2]);
            if (dist < a.high * var && im < backgroundGaussians) bBackgroundHigh = true;
            if (dist < a.low * var) {
              bFitsPDF = true, matched = true;
              const float k = div_rn(Alpha, weight);
              weight = fOneMinAlpha * weight + Alpha;
              g[im][MU] = g[im][MU] - k * (d[0]);
              g[im][MU + 1] = g[im][MU + 1] - k * (d[1]);
              g[im][MU + 2] = g[im][MU + 2] - k * (d[2]);
              const float sigmanew = var + k * (dist - var);
              g[im][VAR] = sigmanew < 4 ? 4 : sigmanew > 5 * m_variance ? 5 * m_variance : sigmanew;
            }
          }
          if (!matched) {  // both of the source's decay branches: the fit was found earlier, or this mode does not fit
            weight = fOneMinAlpha * weight;
            if (weight < 0.0f) weight = 0.0f, nModes--;
          }
          g[im][WEIGHT] = weight;
          totalWeight += weight;
        }
      }
      // weight *= (float)inv; significants = weight / sqrt(variance), for every mode below the count
      auto renormalise = [&](double inv) {
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (k < nModes) {
            g[k][WEIGHT] *= (float)inv;
            sig[k] = div_rn(g[k][WEIGHT], sqrt_rn(g[k][VAR]));
          }
      };
      // stable insertion by adjacent swaps, largest `significants` first (qsort + compareT2FGMM; glibc's qsort keeps equal keys in order)
      auto sort_modes = [&]() {
#pragma unroll
        for (int i2 = 1; i2 < K; ++i2)
          if (i2 < nModes) {
            bool stop = false;
#pragma unroll
            for (int j = i2; j > 0; --j)
              if (!stop) {
                if (sig[j - 1] < sig[j])
                  swap_modes(j - 1, j);
                else
                  stop = true;
              }
          }
      };
      renormalise(1.0 / (double)totalWeight);
      sort_modes();
      if (!bFitsPDF) {
        if (nModes < K) nModes++;  // else: the weakest mode (the last one) is replaced
        const int last = nModes - 1;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (k == last) {
            g[k][MU] = px[0], g[k][MU + 1] = px[1], g[k][MU + 2] = px[2];
            g[k][VAR] = m_variance;
            sig[k] = 0;
            g[k][WEIGHT] = nModes == 1 ? 1.0f : Alpha;
          }
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (k < nModes) sum += g[k][WEIGHT];
        renormalise(1.0 / (double)sum);
      }
      sort_modes();  // the second qsort runs whether or not a mode was added (:292)
      mask = bBackgroundHigh ? 0 : 255;
      nUsed = max(nUsed, nModes);
    }
    dp_store_mask(a, gp, active, mask, t);
  }
  if (active) {
    // a slot that was not loaded is written if it was in use at the end of ANY frame of the launch (see dp_gmm_kernel)
    if (nModes != nLoaded) *pn = (uint8_t)nModes;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int f = 0; f < F; ++f)
        if (k < nLoaded ? __float_as_uint(g[k][f]) != g0[k][f] : k < nUsed) st[(k * F + f) * kDpTile] = g[k][f];
  }
}

}  // namespace bgs
