// engine_t2f.h — host side of package_bgs/tb T2FGMM_UM / T2FGMM_UV (BGS_T2FGMM_UM / BGS_T2FGMM_UV; kernel_t2f.h); included inside
// bgs_hip.hip's anonymous namespace.
//
// The wrapper re-reads its XML on every frame, but the five values reach the model object once, `if(firstTime)`
// (T2FGMM_UM.cpp:45-67): they are taken when the geometry is set and a later bgs_set_t2f_params leaves them in force.  They travel
// the way the wrapper sends them: double threshold / alpha and float km / kv through T2FGMMParams' float& accessors, HighThreshold =
// 2 * LowThreshold in float.

struct T2fState : FamilyState {
  DevPtr<float> planes;    // gaussians * 5 float planes {variance, muR, muG, muB, weight} per mode, tiled over the global pixel index (kernel_dp.h)
  DevPtr<uint8_t> nmodes;  // the mode count per pixel [S][n]
  int K = 0;
  float low = 0, high = 0, alpha = 0, km = 0, kv = 0;  // what the model object was initialised with
};
T2fState& t2f_of(const bgs_engine* e) { return state_of<T2fState>(e); }

const char* t2f_name(bgs_algo a) { return a == BGS_T2FGMM_UM ? "T2FGMM_UM" : "T2FGMM_UV"; }

void t2f_defaults(bgs_t2f_params* p) {  // T2FGMM_UM.cpp:19, T2FGMM_UV.cpp:19
  std::memset(p, 0, sizeof(*p));
  p->struct_size = (uint32_t)sizeof(*p);
  p->threshold = 9.0, p->alpha = 0.01, p->km = 1.5f, p->kv = 0.6f, p->gaussians = 3;
}

// Needs no device: checked before the GPU is opened.
int t2f_check(bgs_algo algo, const bgs_t2f_params& p) {
  const char* nm = t2f_name(algo);
  if (p.gaussians < 1 || p.gaussians > 5) return fail(BGS_ERR_UNSUPPORTED, "%s: the kernels are built for 1..5 gaussians, got %d", nm, p.gaussians);
  if (!std::isfinite((float)p.threshold) || !std::isfinite((float)p.alpha) || !std::isfinite(p.km) || !std::isfinite(p.kv))
    return fail(BGS_ERR_UNSUPPORTED, "%s: threshold %g, alpha %g, km %g, kv %g must all be finite as floats", nm, p.threshold, p.alpha, (double)p.km, (double)p.kv);
  // alpha >= 1 lets every weight decay to 0 (1 / totalWeight = inf, NaN sort keys, on which compareT2FGMM is no order: qsort's result
  // is then its implementation's), alpha < 0 makes the source's `weight < 0` branch live; neither is pinned by any fixture
  if (!((float)p.alpha >= 0.0f && (float)p.alpha < 1.0f)) return fail(BGS_ERR_UNSUPPORTED, "%s: alpha %g is outside [0, 1) as a float", nm, p.alpha);
  if (algo == BGS_T2FGMM_UV && p.kv == 0.0f) return fail(BGS_ERR_UNSUPPORTED, "%s: kv 0 (the distance's factor 1/(kv*kv) - kv*kv is infinite)", nm);
  return BGS_OK;
}
int t2f_check_geometry(bgs_algo algo, int, int, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "%s reads RgbImage pixels: 3-channel frames only (dp/Image.h:257-265)", t2f_name(algo));
  return BGS_OK;
}

int t2f_allocate(bgs_engine* e) {
  const bgs_t2f_params& p = e->t2f;  // the defaults or what passed t2f_check in bgs_set_t2f_params: nothing to refuse here
  const size_t P = e->n * e->S;
  T2fState& st = make_state<T2fState>(e);
  st.K = p.gaussians;
  st.low = (float)p.threshold, st.high = 2 * st.low;  // params.LowThreshold() = threshold; params.HighThreshold() = 2*params.LowThreshold()
  st.alpha = (float)p.alpha, st.km = p.km, st.kv = p.kv;
  DMALLOC(st.nmodes, P);
  const size_t tiles = (P + bgs::kDpTile - 1) / bgs::kDpTile, bytes = tiles * (size_t)(st.K * 5) * bgs::kDpTile * sizeof(float);
  // Nothing is initialised here: InitModel runs in t2f_process at a stream's first frame, on the launch stream (see dp_allocate).
  return model_allocate(e, st.planes, bytes);
}

uint64_t t2f_key(const bgs_engine* e, int i) { return e->seen[i] == 0; }

// `frames` consecutive frames for streams [first, first+count); slab: pixels from one frame of a clip to the next
int t2f_process(bgs_engine* e, int first, int count, int frames, size_t slab, const uint8_t* d_frames, uint8_t* d_fg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const T2fState& st = t2f_of(e);
  bgs::T2fArgs ta{};
  bgs::DpArgs& a = ta.d;
  a = dp_args(e, first, count, frames, slab, d_frames, st.planes, st.nmodes, d_fg, d_bits);
  a.low = st.low, a.high = st.high, a.alpha = st.alpha;
  ta.km = st.km, ta.kv = st.kv;
  const unsigned blocks = blocks_for(a.npix);
  if (e->seen[first] == 0)  // InitModel: every mode field and every count 0 (T2FGMM.cpp:86-99)
    hipLaunchKernelGGL(bgs::dp_gmm_clear_kernel, dim3(blocks), dim3(bgs::kBlock), 0, s, a, st.K * 5);
  Timed tm(e, s, frames > 1 ? "t2f_gmm_kernel (clip: the model stays in registers)" : "t2f_gmm_kernel");
  dp_launch_gmm<bgs::T2fModel>(st.K, e->algo == BGS_T2FGMM_UV, blocks, s, ta);
  *flags = BGS_FG_VALID;  // img_bgmodel is never written by the wrappers
  return BGS_OK;
}

int t2f_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t*, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  return t2f_process(e, first, count, 1, e->n * count, d_frames, d_fg, d_bits, s, flags);
}

int t2f_clip_fused(bgs_engine* e, int first, int count, int fuse, size_t slab, const uint8_t* fr, uint8_t* fg, uint8_t*, uint64_t* bits, hipStream_t s, uint32_t* flags) {
  return t2f_process(e, first, count, fuse, slab, fr, fg, bits, s, flags);
}

// "modes": [K*6][n] floats in the source's struct order {variance, muR, muG, muB, weight, significants}; the sixth is not stored
// (kernel_t2f.h) and is recomputed here for the modes below the pixel's count, 0 above it.  "nmodes": [n] bytes.
int64_t t2f_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const T2fState& st = t2f_of(e);
  const size_t n = e->n;
  if (!strcmp(plane, "nmodes")) return copy_plane(plane, dst, cap, st.nmodes + n * stream, n);
  if (strcmp(plane, "modes")) return unknown_plane(e, plane);
  const int K = st.K;
  if (cap < (size_t)K * 6 * n * 4) return too_small(plane);
  DpTiles tiles;
  std::vector<uint8_t> cnt(n);
  if (dp_fetch_tiles(e, stream, K * 5, st.planes, &tiles) || fetch(cnt.data(), st.nmodes + n * stream, n)) return BGS_ERR_HIP;
  float* out = (float*)dst;
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < K; ++k) {
      for (int f = 0; f < 5; ++f) out[(size_t)(k * 6 + f) * n + i] = tiles.at(k * 5 + f, i);
      const float var = tiles.at(k * 5, i), w = tiles.at(k * 5 + 4, i);
      out[(size_t)(k * 6 + 5) * n + i] = k < cnt[i] ? w / std::sqrt(var) : 0.0f;  // float sqrt and divide, as the source's
    }
  return (int64_t)K * 6 * n * 4;
}

constexpr Family kT2f = [] {
  Family f{};
  f.check_geometry = t2f_check_geometry, f.allocate = t2f_allocate, f.key = t2f_key, f.run = t2f_run, f.get_state = t2f_get_state;
  f.clip_fused = t2f_clip_fused;
  return f;
}();
// frozen: the model object exists once the geometry is set and keeps what it was built with (T2FGMM_UM.cpp `if(firstTime)`)
constexpr ParamBlock<bgs_t2f_params> kT2fBlock{&bgs_engine::t2f, &kT2f, "bgs_t2f_params", "T2FGMM_UM / T2FGMM_UV", t2f_defaults, t2f_check, false};
