// engine_dp.h — host side of the package_bgs/dp/ models (kernel_dp.h); included inside bgs_hip.hip's anonymous namespace.

struct DpState : FamilyState {
  DevPtr<float> planes;     // dp_planes_of() float planes, tiled over the global pixel index (kernel_dp.h); none for AdaptiveMedian
  DevPtr<uint8_t> nmodes;   // the GMMs' mode count per pixel [S][n]
  DevPtr<uint8_t> median;   // AdaptiveMedian's image [S][n*3]
};
DpState& dp_of(const bgs_engine* e) { return state_of<DpState>(e); }

int dp_planes_of(const bgs_engine* e) {
  switch (e->algo) {
    case BGS_DP_ZIVKOVIC_AGMM: return e->p.dp_gaussians * 5;
    case BGS_DP_GRIMSON_GMM: return e->p.dp_gaussians * 6;
    case BGS_DP_WREN_GA: return 4;
    case BGS_DP_MEAN: return 3;
    default: return 0;
  }
}

// calls fn(std::integral_constant<int, K>) for the 1..5 gaussians the tiled GMM kernels are built for (dp_check, t2f_check)
template <class Fn>
void dp_for_gaussians(int K, Fn fn) {
  switch (K) {
    case 1: fn(std::integral_constant<int, 1>()); break;
    case 2: fn(std::integral_constant<int, 2>()); break;
    case 3: fn(std::integral_constant<int, 3>()); break;
    case 4: fn(std::integral_constant<int, 4>()); break;
    default: fn(std::integral_constant<int, 5>()); break;
  }
}

// dp_gmm_kernel<K, Model<second>>: Model = bgs::DpGmmModel (Zivkovic / Grimson) or bgs::T2fModel (UM / UV)
template <template <bool> class Model, class Args>
void dp_launch_gmm(int K, bool second, unsigned blocks, hipStream_t s, const Args& args) {
  dp_for_gaussians(K, [&](auto k) {
    auto kernel = second ? bgs::dp_gmm_kernel<decltype(k)::value, Model<true>> : bgs::dp_gmm_kernel<decltype(k)::value, Model<false>>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(bgs::kBlock), 0, s, args);
  });
}

// what every launch on the tiled state is told: `frames` frames for streams [first, first+count), slab = pixels from one frame of a
// clip to the next; the thresholds, alpha and update are the caller's
bgs::DpArgs dp_args(const bgs_engine* e, int first, int count, int frames, size_t slab, const uint8_t* d_frames, float* planes, uint8_t* bstate, uint8_t* d_fg, uint64_t* d_bits) {
  bgs::DpArgs a{};
  a.frames = frames, a.frame_stride = slab * 3, a.fg_stride = slab, a.bits_stride = slab / 64;
  a.frame = d_frames, a.state = planes, a.bstate = bstate, a.fg = d_fg, a.fg_bits = d_bits;
  a.n = e->n, a.npix = e->n * count, a.first = first;
  a.xcd_swizzle = e->knob.xcd_swizzle;
  return a;
}

int dp_check(bgs_algo algo, const bgs_params& p) {
  if ((algo == BGS_DP_ZIVKOVIC_AGMM || algo == BGS_DP_GRIMSON_GMM) && (p.dp_gaussians < 1 || p.dp_gaussians > 5))
    return fail(BGS_ERR_UNSUPPORTED, "dp GMM kernels are built for 1..5 gaussians, got %d", p.dp_gaussians);
  if (algo == BGS_DP_ADAPTIVE_MEDIAN && p.dp_sampling_rate == 0) return fail(BGS_ERR_UNSUPPORTED, "AdaptiveMedian samplingRate 0 (frame_num %% 0)");
  // DPMeanBGS / DPAdaptiveMedianBGS hold `int threshold`: dp_threshold stands for that int (dp_thresholds below)
  if ((algo == BGS_DP_MEAN || algo == BGS_DP_ADAPTIVE_MEDIAN) && !(p.dp_threshold >= -2147483648.0f && p.dp_threshold < 2147483648.0f))
    return fail(BGS_ERR_UNSUPPORTED, "%s threshold is an int in the reference, got %g", algo == BGS_DP_MEAN ? "DPMeanBGS" : "DPAdaptiveMedianBGS", (double)p.dp_threshold);
  return BGS_OK;
}

// LowThreshold / HighThreshold in the types of the reference's params classes, through which the wrappers pass `threshold`
// (high = 2 * low in that type).  Zivkovic / Grimson / Wren: float.  Mean: unsigned int (MeanBGS.h:50-60) - a negative int wraps,
// and `dist > high` converts high to float.  AdaptiveMedian: unsigned char (AdaptiveMedianBGS.h:50-58) - the int is cut to a byte
// and 2 * low to a byte again (130 -> high 4).  Both integer results are exact as floats where the kernels compare them.
void dp_thresholds(bgs_algo algo, float threshold, float* low, float* high) {
  if (algo == BGS_DP_MEAN) {
    const unsigned lo = (unsigned)(int)threshold, hi = 2u * lo;
    *low = (float)lo, *high = (float)hi;
  } else if (algo == BGS_DP_ADAPTIVE_MEDIAN) {
    const unsigned char lo = (unsigned char)(int)threshold, hi = (unsigned char)(2 * lo);
    *low = lo, *high = hi;
  } else {
    *low = threshold, *high = 2 * threshold;
  }
}

bool dp_is_gmm(const bgs_engine* e) { return e->algo == BGS_DP_ZIVKOVIC_AGMM || e->algo == BGS_DP_GRIMSON_GMM; }

int dp_allocate(bgs_engine* e) {
  if (e->ch != 3) return fail(BGS_ERR_UNSUPPORTED, "the dp/ models read RgbImage pixels: 3-channel frames only (dp/Image.h:257-265)");
  const size_t P = e->n * e->S;
  const int planes = dp_planes_of(e);
  DpState& st = make_state<DpState>(e);
  if (dp_is_gmm(e)) DMALLOC(st.nmodes, P);
  if (e->algo == BGS_DP_ADAPTIVE_MEDIAN) DMALLOC(st.median, P * 3);
  if (planes) {
    const size_t tiles = (P + bgs::kDpTile - 1) / bgs::kDpTile, bytes = tiles * planes * bgs::kDpTile * sizeof(float);
    int rc = model_allocate(e, st.planes, bytes);  // chunked placement for multi-GB models (bgs_hip.hip)
    if (rc) return rc;
  }
  // Nothing is initialised here: InitModel runs in dp_process at a stream's first frame, on the launch stream (an
  // allocation-time memset on another stream is not ordered before a kernel on the caller's / a non-blocking stream).
  return BGS_OK;
}

uint64_t dp_key(const bgs_engine* e, int i) {
  const int64_t t = e->seen[i];
  if (e->algo == BGS_DP_ADAPTIVE_MEDIAN) return (uint64_t)(t == 0) | (uint64_t)((t % e->p.dp_sampling_rate) == 1) << 1;
  return t == 0;
}

// `frames` frames for streams [first, first+count), the first one number e->seen[first] (0-based = the wrappers' frameNumber)
// frames > 1 (Zivkovic / Grimson only, from process_clip): that many consecutive frames in one launch, d_* point at the first
// slab: pixels from one frame of a clip to the next (a single frame: the run is the whole slab)
int dp_process(bgs_engine* e, int first, int count, int frames, size_t slab, const uint8_t* d_frames, uint8_t* d_fg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const DpState& st = dp_of(e);
  const int64_t t = e->seen[first];
  bgs::DpArgs a = dp_args(e, first, count, frames, slab, d_frames, st.planes, dp_is_gmm(e) ? st.nmodes : st.median, d_fg, d_bits);
  dp_thresholds(e->algo, p.dp_threshold, &a.low, &a.high);  // HighThreshold = 2*LowThreshold, e.g. DPZivkovicAGMMBGS.cpp:58
  a.alpha = p.dp_alpha;
  const unsigned blocks = blocks_for(a.npix);
  if (t == 0 && (e->algo == BGS_DP_ZIVKOVIC_AGMM || e->algo == BGS_DP_GRIMSON_GMM))  // InitModel: all modes and counts 0
    hipLaunchKernelGGL(bgs::dp_gmm_clear_kernel, dim3(blocks), dim3(bgs::kBlock), 0, s, a, dp_planes_of(e));
  if (t == 0 && (e->algo == BGS_DP_WREN_GA || e->algo == BGS_DP_MEAN))  // InitModel from the first frame
    hipLaunchKernelGGL(bgs::dp_init_kernel, dim3(blocks), dim3(bgs::kBlock), 0, s, a, e->algo == BGS_DP_WREN_GA ? 4 : 3, 36.0f);
  if (t == 0 && e->algo == BGS_DP_ADAPTIVE_MEDIAN)
    HIP_TRY(hipMemcpyAsync(st.median + (size_t)first * e->n * 3, d_frames, a.npix * 3, hipMemcpyDeviceToDevice, s));
  switch (e->algo) {
    case BGS_DP_ZIVKOVIC_AGMM:
    case BGS_DP_GRIMSON_GMM: {
      Timed tm(e, s, "dp_gmm_kernel");
      dp_launch_gmm<bgs::DpGmmModel>(p.dp_gaussians, e->algo == BGS_DP_GRIMSON_GMM, blocks, s, a);
      break;
    }
    case BGS_DP_WREN_GA: {
      Timed tm(e, s, "dp_wren_kernel");
      hipLaunchKernelGGL(bgs::dp_wren_kernel, dim3(blocks), dim3(bgs::kBlock), 0, s, a);
      break;
    }
    case BGS_DP_MEAN: {
      Timed tm(e, s, "dp_mean_kernel");
      hipLaunchKernelGGL(bgs::dp_mean_kernel, dim3(blocks), dim3(bgs::kBlock), 0, s, a);
      break;
    }
    default: {
      a.update = (t % p.dp_sampling_rate) == 1;  // AdaptiveMedianBGS.cpp:60
      Timed tm(e, s, "dp_median_kernel");
      const uint8_t* med0 = st.median + (size_t)first * e->n * 3;
      if (a.npix % 4 == 0 && aligned(d_frames, 4) && aligned(med0, 4) && (!d_fg || aligned(d_fg, 4)))
        hipLaunchKernelGGL((bgs::dp_median_kernel<4>), dim3(blocks_for(a.npix / 4)), dim3(bgs::kBlock), 0, s, a);
      else
        hipLaunchKernelGGL((bgs::dp_median_kernel<1>), dim3(blocks), dim3(bgs::kBlock), 0, s, a);
      break;
    }
  }
  *flags = BGS_FG_VALID;  // img_bgmodel is never written by the dp wrappers
  return BGS_OK;
}

int dp_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t*, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  return dp_process(e, first, count, 1, e->n * count, d_frames, d_fg, d_bits, s, flags);
}

// package_bgs/dp GMMs: the same kernel with a frame loop (kernel_dp.h)
int dp_clip_fused(bgs_engine* e, int first, int count, int fuse, size_t slab, const uint8_t* fr, uint8_t* fg, uint8_t*, uint64_t* bits, hipStream_t s, uint32_t* flags) {
  return dp_process(e, first, count, fuse, slab, fr, fg, bits, s, flags);
}

// the tiles of a tiled state of `planes` planes (kernel_dp.h) that hold one stream, fetched to the host
struct DpTiles {
  std::vector<float> tiles;
  size_t g0, t0, TF;
  float at(int plane, size_t i) const {
    const size_t g = g0 + i, T = bgs::kDpTile;
    return tiles[(g / T - t0) * TF + (size_t)plane * T + g % T];
  }
};
int dp_fetch_tiles(const bgs_engine* e, int stream, int planes, const float* d_planes, DpTiles* out) {
  const size_t n = e->n, T = bgs::kDpTile;
  out->g0 = (size_t)stream * n, out->t0 = out->g0 / T, out->TF = (size_t)planes * T;
  out->tiles.resize(((out->g0 + n - 1) / T + 1 - out->t0) * out->TF);
  return fetch(out->tiles.data(), d_planes + out->t0 * out->TF, out->tiles.size() * 4);
}

// canonical export [plane][n] of one stream from the tiled device layout
int64_t dp_export_planes(bgs_engine* e, int stream, int planes, void* dst, size_t cap) {
  const size_t n = e->n;
  if (cap < (size_t)planes * n * 4) return fail(BGS_ERR_STATE, "buffer too small for %d planes", planes);
  DpTiles tiles;
  if (dp_fetch_tiles(e, stream, planes, dp_of(e).planes, &tiles)) return BGS_ERR_HIP;
  for (int q = 0; q < planes; ++q)
    for (size_t i = 0; i < n; ++i) ((float*)dst)[(size_t)q * n + i] = tiles.at(q, i);
  return (int64_t)planes * n * 4;
}

// planes are stored canonically: [stream][plane][n]
int64_t dp_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t n = e->n, off = n * stream;
  const int planes = dp_planes_of(e);
  const char* fname = (e->algo == BGS_DP_WREN_GA) ? "gauss" : (e->algo == BGS_DP_MEAN) ? "mean" : "modes";
  if (planes && !strcmp(plane, fname)) return dp_export_planes(e, stream, planes, dst, cap);
  if (dp_is_gmm(e) && !strcmp(plane, "nmodes")) return copy_plane(plane, dst, cap, dp_of(e).nmodes + off, n);
  if (e->algo == BGS_DP_ADAPTIVE_MEDIAN && !strcmp(plane, "median")) return copy_plane(plane, dst, cap, dp_of(e).median + off * 3, n * 3);
  return unknown_plane(e, plane);
}

// handed to the model object once, when it is built on the first frame (DP*BGS.cpp `if(firstTime)`)
void dp_keep_frozen(bgs_params& p, const bgs_params& old) {
  p.dp_threshold = old.dp_threshold, p.dp_alpha = old.dp_alpha, p.dp_gaussians = old.dp_gaussians;
  p.dp_sampling_rate = old.dp_sampling_rate, p.learning_frames = old.learning_frames;
}

constexpr Family kDp = [] {
  Family f{};
  f.check = dp_check, f.allocate = dp_allocate, f.key = dp_key, f.run = dp_run, f.get_state = dp_get_state;
  f.keep_frozen = dp_keep_frozen, f.clip_fused = dp_clip_fused, f.clip_fusable = dp_is_gmm;
  return f;
}();
