// kernel_eigen.h — package_bgs/dp DPEigenbackgroundBGS (BGS_DP_EIGENBACKGROUND, USTC_BGS type 15) for gfx950: a PCA background over
// whole frames (dp/Eigenbackground.cpp).  Host side: engine_eigen.h; numeric contract: DESIGN.md §5.9.
//
// A frame is one vector of L = 3 n bytes.  Frames 0 .. H-1 are stored (eigen_store_kernel); in front of frame H's detection the model
// is built once - the integer Gram matrix of the H stored frames (eigen_gram_kernel), its centring and eigen-decomposition
// (eigen_solve_kernel), the M eigenvectors of the 3n x 3n covariance as linear combinations of the centred frames
// (eigen_basis_kernel) - and every frame from H on is projected onto them (eigen_project_kernel, eigen_coeff_kernel) and compared with
// its reconstruction (eigen_reconstruct_kernel).
//
// Layout per stream: the history [H][Lp] bytes, avg [Lp] floats, the eigenvectors [M][Lp] floats, Lp = L rounded up to 4 so that
// every history row starts on a dword; the pad bytes of the history are zero, so they add nothing to any sum.
//
// No float atomics anywhere: the only atomics add exact integers (the Gram matrix), every float sum has a fixed order, and a stream's
// chunking depends on its own n alone - a stream's bytes do not depend on which launch it shares with whom (Guideline 12).
#pragma once
#include "bgs_device.h"

namespace bgs {

constexpr int kEigMaxH = 32;          // BGS_EIGEN_MAX_HISTORY
constexpr int kEigGramChunk = 4096;   // dwords of every history row per workgroup: a 32-bit partial takes 4096 dot4 of at most 260 100 each = 1.07e9 (it would wrap after 16 512)
constexpr int kEigGramTile = 64;      // dwords of every history row staged in LDS at a time
constexpr int kEigChunk = 8192;       // elements per projection chunk: one workgroup, one slab entry per eigenvector
constexpr int kEigRows = 8;           // eigenvectors accumulated per pass over a chunk

struct EigenArgs {
  const uint8_t* cur;        // [count][L] the run's frames (null: eigen_reconstruct_kernel only writes `result`)
  uint8_t* fg;               // [count][n] or null
  uint64_t* bits;            // [count][n / 64] or null (n % 64 == 0)
  float* result;             // [L] or null: the reconstruction itself (bgs_get_state "result"; count == 1)
  // the state of the run's first stream; stream k of the run follows at k times the per-stream size
  uint8_t* hist;             // [H][Lp]
  float* avg;                // [Lp]
  float* E;                  // [M][Lp]
  unsigned long long* G;     // [H][H] raw integer Gram matrix, entries s <= t
  double* W;                 // [M][H] V[.][i] / sqrt(lambda_i)
  double* lam;               // [H] eigenvalues of the centred Gram matrix, descending
  double* slab;              // [chunks][M] partial projections
  float* coeff;              // [M]
  uint32_t n, L, Lp, H, M, chunks;
  float high;                // 2 * (float)threshold
};

// Frames 0 .. H-1: the frame goes into history row `slot` (pad bytes zero), the mask is all background.
__global__ __launch_bounds__(kBlock) void eigen_store_kernel(EigenArgs a, uint32_t slot) {
  const uint32_t k = blockIdx.y, j = blockIdx.x * kBlock + threadIdx.x;
  if (j < a.Lp) a.hist[((size_t)k * a.H + slot) * a.Lp + j] = j < a.L ? a.cur[(size_t)k * a.L + j] : (uint8_t)0;
  if (a.fg && j < a.n) a.fg[(size_t)k * a.n + j] = 0;
  if (a.bits && j < a.n / 64) a.bits[(size_t)k * (a.n / 64) + j] = 0;
}

// G[s][t] += sum over this workgroup's dwords of dot4(X[s], X[t]) for s <= t.  Integer sums: exact, so the order the workgroups'
// 64-bit atomics arrive in does not matter.  H (H + 1) / 2 <= 528 pairs over 256 threads: at most three pairs per thread.
__global__ __launch_bounds__(kBlock) void eigen_gram_kernel(EigenArgs a) {
  __shared__ uint32_t tile[kEigMaxH][kEigGramTile + 1];
  const uint32_t k = blockIdx.y, H = a.H, D = a.Lp >> 2, P = H * (H + 1) / 2;
  const uint32_t* X = reinterpret_cast<const uint32_t*>(a.hist + (size_t)k * H * a.Lp);
  const uint32_t d0 = blockIdx.x * kEigGramChunk, d1 = min(D, d0 + (uint32_t)kEigGramChunk);
  uint32_t ps[3], pt[3], acc[3] = {0, 0, 0};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    uint32_t rem = threadIdx.x + q * kBlock, s = 0;
    if (rem >= P) rem = 0;  // no pair: computes pair 0 and drops it
    while (rem >= H - s) rem -= H - s, ++s;
    ps[q] = s, pt[q] = s + rem;
  }
  for (uint32_t base = d0; base < d1; base += kEigGramTile) {
    const uint32_t w = min((uint32_t)kEigGramTile, d1 - base);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < H * kEigGramTile; i += kBlock) {
      const uint32_t r = i / kEigGramTile, c = i % kEigGramTile;
      tile[r][c] = c < w ? X[(size_t)r * D + base + c] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (threadIdx.x + q * kBlock >= P) continue;
      uint32_t v = acc[q];
#pragma unroll 8
      for (int c = 0; c < kEigGramTile; ++c) v = __builtin_amdgcn_udot4(tile[ps[q]][c], tile[pt[q]][c], v, false);
      acc[q] = v;
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (threadIdx.x + q * kBlock < P) atomicAdd(&a.G[((size_t)k * H + ps[q]) * H + pt[q]], (unsigned long long)acc[q]);
}

// One wave per stream.  Centres G exactly in integers (A = H^2 G - H (r_s + r_t) + T, r the row sums of G, T the sum of all of it;
// Gc = A / H^2), runs cyclic Jacobi in double in a fixed rotation order until the off-diagonal mass is at most 2^-52 of the trace or
// 30 sweeps have run, sorts the eigenpairs descending (ties keep index order) and writes W[i][.] = V[.][i] / sqrt(lambda_i), all
// zero where lambda_i <= H 2^-40 lambda_0 - what cv::normalize makes of a zero vector.
__global__ __launch_bounds__(kWave) void eigen_solve_kernel(EigenArgs a) {
  __shared__ double A[kEigMaxH][kEigMaxH + 1], V[kEigMaxH][kEigMaxH + 1], lam[kEigMaxH];
  __shared__ long long rs[kEigMaxH];
  __shared__ int ord[kEigMaxH];
  const uint32_t k = blockIdx.x, H = a.H, M = a.M, lane = threadIdx.x;
  const unsigned long long* g = a.G + (size_t)k * H * H;
  auto G = [&](uint32_t s, uint32_t t) { return (long long)(s <= t ? g[s * H + t] : g[t * H + s]); };
  if (lane < H) {
    long long r = 0;
    for (uint32_t t = 0; t < H; ++t) r += G(lane, t);
    rs[lane] = r;
  }
  __syncthreads();
  long long T = 0;
  for (uint32_t s = 0; s < H; ++s) T += rs[s];
  const long long h = (long long)H;
  if (lane < H)
    for (uint32_t t = 0; t < H; ++t) {
      const long long c = h * h * G(lane, t) - h * (rs[lane] + rs[t]) + T;
      A[lane][t] = (double)c / (double)(h * h);
      V[lane][t] = lane == t ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {
    __syncthreads();
    double off = 0, tr = 0;  // every lane the same sums in the same order: the exit is uniform
    for (uint32_t p = 0; p < H; ++p) {
      tr += A[p][p];
      for (uint32_t q = p + 1; q < H; ++q) off += A[p][q] * A[p][q];
    }
    if (sqrt(off) <= 0x1p-52 * tr) break;
    for (uint32_t p = 0; p + 1 < H; ++p)
      for (uint32_t q = p + 1; q < H; ++q) {
        const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
        if (apq == 0.0) continue;  // uniform
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        __syncthreads();
        if (lane < H) {  // A J and V J: columns p and q
          const double aip = A[lane][p], aiq = A[lane][q], vip = V[lane][p], viq = V[lane][q];
          A[lane][p] = c * aip - s * aiq, A[lane][q] = s * aip + c * aiq;
          V[lane][p] = c * vip - s * viq, V[lane][q] = s * vip + c * viq;
        }
        __syncthreads();
        if (lane < H) {  // J^T (A J): rows p and q
          const double apj = A[p][lane], aqj = A[q][lane];
          A[p][lane] = c * apj - s * aqj, A[q][lane] = s * apj + c * aqj;
        }
        __syncthreads();
        if (lane == 0) A[p][q] = 0.0, A[q][p] = 0.0;
        __syncthreads();
      }
  }
  __syncthreads();
  if (lane < H) lam[lane] = A[lane][lane];
  __syncthreads();
  if (lane == 0)  // insertion sort, descending, stable
    for (uint32_t i = 0; i < H; ++i) {
      int j = (int)i;
      while (j > 0 && lam[ord[j - 1]] < lam[i]) ord[j] = ord[j - 1], --j;
      ord[j] = (int)i;
    }
  __syncthreads();
  if (lane < H) {
    a.lam[(size_t)k * H + lane] = lam[ord[lane]];
    const double l0 = lam[ord[0]];
    for (uint32_t i = 0; i < M; ++i) {
      const double li = lam[ord[i]];
      a.W[((size_t)k * M + i) * H + lane] = li <= (double)H * 0x1p-40 * l0 ? 0.0 : V[lane][ord[i]] / sqrt(li);
    }
  }
}

// avg[j] = (float)S[j] / (float)H and E_i[j] = (float) sum_t W[i][t] ((double)X[t][j] - (double)S[j] / H), t in index order; no
// renormalisation.  One lane per element, pad elements included (they come out 0).
__global__ __launch_bounds__(kBlock) void eigen_basis_kernel(EigenArgs a) {
  __shared__ double W[(kEigMaxH - 1) * kEigMaxH];
  const uint32_t k = blockIdx.y, H = a.H, M = a.M, j = blockIdx.x * kBlock + threadIdx.x;
  for (uint32_t i = threadIdx.x; i < M * H; i += kBlock) W[i] = a.W[(size_t)k * M * H + i];
  __syncthreads();
  if (j >= a.Lp) return;
  const uint8_t* X = a.hist + (size_t)k * H * a.Lp + j;
  double xc[kEigMaxH];
  uint32_t S = 0;
#pragma unroll
  for (int t = 0; t < kEigMaxH; ++t) {
    const uint32_t x = t < (int)H ? X[(size_t)t * a.Lp] : 0u;
    S += x, xc[t] = (double)x;
  }
  const double mean = (double)S / (double)H;
  a.avg[(size_t)k * a.Lp + j] = (float)S / (float)H;
#pragma unroll
  for (int t = 0; t < kEigMaxH; ++t) xc[t] -= mean;
  for (uint32_t i = 0; i < M; ++i) {
    double acc = 0;
#pragma unroll
    for (int t = 0; t < kEigMaxH; ++t)
      if (t < (int)H) acc += W[i * H + t] * xc[t];
    a.E[((size_t)k * M + i) * a.Lp + j] = (float)acc;
  }
}

// Four consecutive frame bytes starting at element j (a multiple of 4) as one dword, byte q in bits 8q..8q+7; elements from L on read
// 0.  One dword load where the frame is dword-aligned and the four bytes are the frame's own, byte loads otherwise: the same value.
__device__ __forceinline__ uint32_t eigen_frame4(const uint8_t* x, uint32_t j, uint32_t L) {
  if ((reinterpret_cast<uintptr_t>(x) & 3) == 0 && j + 4 <= L) return *reinterpret_cast<const uint32_t*>(x + j);
  uint32_t w = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (j + q < L) w |= (uint32_t)x[j + q] << (8 * q);
  return w;
}

// slab[chunk][i] = sum over the chunk's elements of ((double)x[j] - (double)avg[j]) (double)E_i[j].  A lane takes four consecutive
// elements at a time (one float4 of avg and of every eigenvector; the pad elements of the last group add 0) and sums in element
// order; then a butterfly over the wave, then the four waves in wave order.
__global__ __launch_bounds__(kBlock) void eigen_project_kernel(EigenArgs a) {
  __shared__ double red[kBlock / kWave][kEigRows];
  const uint32_t k = blockIdx.y, M = a.M, chunk = blockIdx.x;
  const uint32_t j0 = chunk * kEigChunk, j1 = min(a.L, j0 + (uint32_t)kEigChunk);
  const uint8_t* x = a.cur + (size_t)k * a.L;
  const float* avg = a.avg + (size_t)k * a.Lp;
  const float* E = a.E + (size_t)k * M * a.Lp;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t i0 = 0; i0 < M; i0 += kEigRows) {
    const int nr = (int)min((uint32_t)kEigRows, M - i0);
    double acc[kEigRows];
#pragma unroll
    for (int u = 0; u < kEigRows; ++u) acc[u] = 0;
    for (uint32_t j = j0 + 4 * threadIdx.x; j < j1; j += 4 * kBlock) {  // j0 is a multiple of 4 and j + 3 < Lp
      const float4 av = *reinterpret_cast<const float4*>(avg + j);
      const uint32_t xw = eigen_frame4(x, j, a.L);
      const double d0 = (double)byte_of(xw, 0) - (double)av.x, d1 = (double)byte_of(xw, 1) - (double)av.y;
      const double d2 = (double)byte_of(xw, 2) - (double)av.z, d3 = (double)byte_of(xw, 3) - (double)av.w;
#pragma unroll
      for (int u = 0; u < kEigRows; ++u)
        if (u < nr) {
          const float4 ev = *reinterpret_cast<const float4*>(E + (size_t)(i0 + u) * a.Lp + j);
          acc[u] += d0 * (double)ev.x, acc[u] += d1 * (double)ev.y, acc[u] += d2 * (double)ev.z, acc[u] += d3 * (double)ev.w;
        }
    }
#pragma unroll
    for (int u = 0; u < kEigRows; ++u)
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) acc[u] += __shfl_xor(acc[u], o, kWave);
    __syncthreads();  // the previous pass's readers are done
    if (lane == 0)
#pragma unroll
      for (int u = 0; u < kEigRows; ++u) red[wave][u] = acc[u];
    __syncthreads();
    if ((int)threadIdx.x < nr) a.slab[((size_t)k * a.chunks + chunk) * M + i0 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  }
}

// coeff[i] = (float) sum of slab[.][i]: lane l takes chunks l, l + 256, ... in index order, then a fixed tree over the 256 lanes.
// The reference's `proj` is CV_32F.
__global__ __launch_bounds__(kBlock) void eigen_coeff_kernel(EigenArgs a) {
  __shared__ double red[kBlock];
  const uint32_t k = blockIdx.x, M = a.M;
  const double* slab = a.slab + (size_t)k * a.chunks * M;
  for (uint32_t i = 0; i < M; ++i) {
    double s = 0;
    for (uint32_t c = threadIdx.x; c < a.chunks; c += kBlock) s += slab[(size_t)c * M + i];
    __syncthreads();
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) a.coeff[(size_t)k * M + i] = (float)red[0];
  }
}

// r[j] = (float)((double)avg[j] + sum_i (double)c_i (double)E_i[j]), i in index order; a pixel is foreground iff for any of its
// three channels ((double)x - (double)r)^2 > (double)high (Eigenbackground.cpp:121-156; the wrapper hands out the high-threshold
// mask).  One workgroup per 256 pixels = 768 consecutive elements, four per lane (float4 loads); the three flags of a pixel meet in LDS.
__global__ __launch_bounds__(kBlock) void eigen_reconstruct_kernel(EigenArgs a) {
  __shared__ float cf[kEigMaxH];
  __shared__ uint32_t flagw[3 * kBlock / 4];  // one byte per element
  const uint8_t* flag = reinterpret_cast<const uint8_t*>(flagw);
  const uint32_t k = blockIdx.y, M = a.M, p0 = blockIdx.x * kBlock;
  const float* avg = a.avg + (size_t)k * a.Lp;
  const float* E = a.E + (size_t)k * M * a.Lp;
  if (threadIdx.x < M) cf[threadIdx.x] = a.coeff[(size_t)k * M + threadIdx.x];
  __syncthreads();
  const double high = (double)a.high;
  if (threadIdx.x < 3 * kBlock / 4) {  // 768 elements = 192 groups of four (768 blockIdx.x is a multiple of 4)
    const uint32_t j = p0 * 3 + 4 * threadIdx.x;
    uint32_t f = 0;
    if (j < a.L) {
      double s[4] = {0, 0, 0, 0};
#pragma unroll 4
      for (uint32_t i = 0; i < M; ++i) {
        const float4 ev = *reinterpret_cast<const float4*>(E + (size_t)i * a.Lp + j);
        const double c = (double)cf[i];
        s[0] += c * (double)ev.x, s[1] += c * (double)ev.y, s[2] += c * (double)ev.z, s[3] += c * (double)ev.w;
      }
      const float4 av = *reinterpret_cast<const float4*>(avg + j);
      const float r[4] = {(float)((double)av.x + s[0]), (float)((double)av.y + s[1]), (float)((double)av.z + s[2]), (float)((double)av.w + s[3])};
      if (a.result)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (j + q < a.L) a.result[j + q] = r[q];
      if (a.cur) {
        const uint32_t xw = eigen_frame4(a.cur + (size_t)k * a.L, j, a.L);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double d = (double)byte_of(xw, q) - (double)r[q];
          f |= (uint32_t)(j + q < a.L && d * d > high) << (8 * q);
        }
      }
    }
    flagw[threadIdx.x] = f;
  }
  __syncthreads();
  const uint32_t p = p0 + threadIdx.x;
  const bool in = p < a.n;
  const bool fgp = in && (flag[3 * threadIdx.x] | flag[3 * threadIdx.x + 1] | flag[3 * threadIdx.x + 2]);
  if (a.fg && in) a.fg[(size_t)k * a.n + p] = fgp ? 255 : 0;
  if (a.bits) {  // n % 64 == 0: a wave's 64 pixels are one word of one stream
    const unsigned long long b = __ballot(fgp);
    if ((threadIdx.x & (kWave - 1)) == 0 && in) a.bits[(size_t)k * (a.n / 64) + p / 64] = b;
  }
}

}  // namespace bgs
