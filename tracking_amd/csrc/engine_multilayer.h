// engine_multilayer.h — host side of package_bgs/jmo MultiLayerBGS (BGS_MULTILAYER; kernel_multilayer.h); included inside
// bgs_hip.hip's anonymous namespace.
//
// The wrapper hands its parameters to CMultiLayerBGS once, at its first frame (MultiLayerBGS.cpp:69-193): they are taken when the
// geometry is set, and a later bgs_set_multilayer_params succeeds and leaves the values in force.  What changes afterwards is the
// switch at detect_after, a function of the stream's frame counter alone, so it is part of the launch key and the host picks the
// rates per run.  Nothing here waits for the device.

struct MlState : FamilyState {
  DevPtr<uint32_t> model;  // [S][kMlPlanes][n]
  DevPtr<float> raw, dist; // [S][n] each
  DevPtr<uint32_t> empty_last;  // [S]: the reference's bFirstFrame of the stream's latest frame (kernel_multilayer.h)
  float k[2 * bgs::kMlMaxHalf + 1] = {1.f};
  int half = 0;
  float min_sine = 0.f;
};
MlState& ml_of(const bgs_engine* e) { return state_of<MlState>(e); }

constexpr const char* kMlName = "MultiLayerBGS";

void ml_defaults(bgs_multilayer_params* p) {  // MultiLayerBGS.cpp:110-186, the loadDefaultParams block; the rest are loadConfig's defaults
  std::memset(p, 0, sizeof(*p));
  p->struct_size = (uint32_t)sizeof(*p);
  p->max_mode_num = 5, p->weight_updating_constant = 5.0f, p->texture_weight = 0.5f, p->bg_mode_percent = 0.6f;
  p->pattern_neig_half_size = 4, p->pattern_neig_gaus_sigma = 3.0f, p->bg_prob_threshold = 0.2f, p->bg_prob_updating_threshold = 0.2f;
  p->robust_LBP_constant = 3;
  p->min_noised_angle = (float)(10.0 / 180.0 * 3.141592653589793f);  // double arithmetic on the float PI macro, stored as float
  p->shadow_rate = 0.6f, p->highlight_rate = 1.2f, p->frame_duration = 1.0f / 10.0f;
  p->learn_mode_learn_rate_per_second = 0.5f, p->learn_weight_learn_rate_per_second = 0.5f, p->learn_init_mode_weight = 0.05f;
  p->detect_mode_learn_rate_per_second = 0.01f, p->detect_weight_learn_rate_per_second = 0.01f, p->detect_init_mode_weight = 0.001f;
  p->status = 0, p->disable_detect_mode = 1, p->disable_learning = 0, p->detect_after = 0;
}

// m_fMinNoisedAngleSine: the constructor's sinf(3 degrees), never recomputed (ResetAllParameters runs before the wrapper assigns)
float ml_min_sine() {
  volatile float three = 3.0f;
  const float angle = three / 180.0f * 3.141592653589793f;
  return sinf(angle);
}

// Needs no device: checked before the GPU is opened.
int ml_check(bgs_algo, const bgs_multilayer_params& p) {
  const float fl[] = {p.weight_updating_constant, p.texture_weight, p.bg_mode_percent, p.pattern_neig_gaus_sigma, p.bg_prob_threshold, p.bg_prob_updating_threshold,
                      p.min_noised_angle, p.shadow_rate, p.highlight_rate, p.frame_duration, p.learn_mode_learn_rate_per_second, p.learn_weight_learn_rate_per_second,
                      p.learn_init_mode_weight, p.detect_mode_learn_rate_per_second, p.detect_weight_learn_rate_per_second, p.detect_init_mode_weight};
  for (float v : fl)
    if (!std::isfinite(v)) return fail(BGS_ERR_UNSUPPORTED, "%s: every parameter must be finite", kMlName);
  if (p.max_mode_num < 1 || p.max_mode_num > bgs::kMlSlots)
    return fail(BGS_ERR_UNSUPPORTED, "%s: max_mode_num %d is outside 1..%d (the reference allocates MAX_LBP_MODE_NUM slots before it learns the number)", kMlName, p.max_mode_num, bgs::kMlSlots);
  if (p.pattern_neig_half_size > BGS_MULTILAYER_MAX_HALF_SIZE)
    return fail(BGS_ERR_UNSUPPORTED, "%s: pattern_neig_half_size %d is above %d (the smoothing tile's halo)", kMlName, p.pattern_neig_half_size, BGS_MULTILAYER_MAX_HALF_SIZE);
  if (p.pattern_neig_half_size >= 0 && !(p.pattern_neig_gaus_sigma > 0))
    return fail(BGS_ERR_UNSUPPORTED, "%s: pattern_neig_gaus_sigma %g must be above 0 when pattern_neig_half_size is not negative", kMlName, p.pattern_neig_gaus_sigma);
  return BGS_OK;
}
int ml_check_geometry(bgs_algo, int, int, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "%s: 3-channel frames only (SetRGBInputImage, CMultiLayerBGS.cpp:2084-2090)", kMlName);
  return BGS_OK;
}

int ml_allocate(bgs_engine* e) {
  const bgs_multilayer_params& p = e->ml;  // the defaults or what passed ml_check in bgs_set_multilayer_params
  const size_t S = (size_t)e->S, n = e->n;
  if (n >= (size_t)1 << 31) return fail(BGS_ERR_INVALID, "%s: an image must stay below 2^31 pixels", kMlName);
  MlState& st = make_state<MlState>(e);
  int rc = model_allocate(e, st.model, S * bgs::kMlPlanes * n * 4);
  if (rc) return rc;
  DMALLOC(st.raw, S * n * 4);
  DMALLOC(st.dist, S * n * 4);
  DMALLOC(st.empty_last, S * 4);
  st.half = p.pattern_neig_half_size > 0 ? p.pattern_neig_half_size : 0;  // below 0: no smoothing; 0: GaussianBlur copies a 1 x 1 kernel
  st.k[0] = 1.f;  // either way the one tap 1.0f leaves every value as it is
  if (st.half > 0) gaussian_kernel_f32(2 * st.half + 1, p.pattern_neig_gaus_sigma, st.k);
  st.min_sine = ml_min_sine();
  // Nothing is initialised here: a stream's first frame clears its headers on the launch stream (ml_run)
  return BGS_OK;
}

bool ml_detecting(const bgs_engine* e, int i) { return e->ml.detect_after > 0 && e->seen[i] >= (int64_t)e->ml.detect_after; }
// a stream's first frame clears its headers; past detect_after the hard-coded DETECT rates are in force
uint64_t ml_key(const bgs_engine* e, int i) { return (e->seen[i] == 0 ? 1u : 0u) | (ml_detecting(e, i) ? 2u : 0u); }

bgs::MlArgs ml_args(const bgs_engine* e, int first, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg) {
  const MlState& st = ml_of(e);
  const bgs_multilayer_params& p = e->ml;
  const size_t f = (size_t)first, n = e->n;
  bgs::MlArgs a{};
  a.cur = d_frames, a.fg = d_fg, a.bgout = d_bg;
  a.model = st.model + f * bgs::kMlPlanes * n, a.raw = st.raw + f * n, a.dist = st.dist + f * n, a.empty_last = st.empty_last + f;
  a.n = (uint32_t)n, a.rows = e->rows, a.cols = e->cols;
  a.max_modes = p.max_mode_num, a.first = e->seen[first] == 0, a.texture = p.texture_weight > 0;
  // the wrapper's status (MultiLayerBGS.cpp:71-108, :156-188) and the switch at detect_after (:200-218)
  const int status0 = p.disable_detect_mode ? 0 : p.status;
  float mode = status0 ? p.detect_mode_learn_rate_per_second : p.learn_mode_learn_rate_per_second;
  float weight = status0 ? p.detect_weight_learn_rate_per_second : p.learn_weight_learn_rate_per_second;
  a.init_w = status0 ? p.detect_init_mode_weight : p.learn_init_mode_weight;
  a.learn = !(status0 && p.disable_learning);
  if (ml_detecting(e, first)) mode = 0.01f, weight = 0.01f, a.init_w = 0.001f, a.learn = !p.disable_learning;  // not the configured detect_* values
  a.mrate = mode * p.frame_duration, a.m1 = 1.0f - a.mrate, a.wrate = weight * p.frame_duration;  // SetParameters
  a.tw = p.texture_weight, a.wc = p.weight_updating_constant, a.percent = p.bg_mode_percent;
  a.thr = p.bg_prob_threshold, a.upd_thr = p.bg_prob_updating_threshold;
  a.offset = std::max((float)p.robust_LBP_constant, 5.0f);  // MAX(m_fRobustColorOffset, 5.0f) in CalColorBgDist; the LBP offset stays 6
  a.min_sine = st.min_sine, a.min_angle = p.min_noised_angle, a.shadow = p.shadow_rate, a.high = p.highlight_rate;
  a.half = st.half;
  std::memcpy(a.k, st.k, sizeof(a.k));
  return a;
}

int ml_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const size_t n = e->n, N = n * (size_t)count;
  const bgs::MlArgs a = ml_args(e, first, d_frames, d_fg, d_bg);
  if (a.first)  // Initialization: num = 0 in every pixel; plane 0 of each stream of the run (the whole run is on its first frame, ml_key)
    HIP_TRY(hipMemset2DAsync(a.model, (size_t)bgs::kMlPlanes * n * 4, 0, n * 4, (size_t)count, s));
  {
    Timed tm(e, s, "ml_model_kernel");
    hipLaunchKernelGGL(bgs::ml_model_kernel, dim3(blocks_for(n), (unsigned)count), dim3(bgs::kBlock), 0, s, a);
  }
  const dim3 tiles((unsigned)((e->cols + bgs::kMlTileW - 1) / bgs::kMlTileW), (unsigned)((e->rows + bgs::kMlTileH - 1) / bgs::kMlTileH), (unsigned)count);
  hipLaunchKernelGGL(bgs::ml_smooth_kernel, tiles, dim3(bgs::kBlock), 0, s, a);
  if (d_bits) hipLaunchKernelGGL(bgs::mask_pack_kernel, dim3(blocks_for(N)), dim3(bgs::kBlock), 0, s, (const uint8_t*)d_fg, d_bits, N);  // n % 64 == 0 here; d_fg: needs_byte_mask
  *flags = BGS_FG_VALID | BGS_BG_VALID;  // the first frame's mask is the reference's zero mask
  return BGS_OK;
}

// bgs_get_state planes (include/bgs_hip.h), unpacked in the reference's field order
int64_t ml_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const MlState& st = ml_of(e);
  const size_t n = e->n, k = (size_t)stream;
  const bool fresh = e->seen[stream] == 0;  // Initialization has not run: what it would leave
  if (!strcmp(plane, "dist")) {
    if (cap < n * 4) return too_small(plane);
    if (fresh) return std::memset(dst, 0, n * 4), (int64_t)(n * 4);
    return copy_plane(plane, dst, cap, st.dist + k * n, n * 4);
  }
  const bool order = !strcmp(plane, "order"), modes = !strcmp(plane, "modes");
  if (!order && !modes) return unknown_plane(e, plane);
  const size_t nb = order ? n * 7 : n * bgs::kMlSlots * 18 * 4;
  if (cap < nb) return too_small(plane);
  std::memset(dst, 0, nb);
  if (fresh) return (int64_t)nb;
  const size_t planes = order ? 1 : bgs::kMlPlanes;
  std::vector<uint32_t> w(planes * n);
  if (fetch(w.data(), st.model + k * bgs::kMlPlanes * n, planes * n * 4)) return BGS_ERR_HIP;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t h = w[i], num = h & 7u;
    if (order) {
      uint8_t* o = (uint8_t*)dst + i * 7;
      o[0] = (uint8_t)num, o[1] = (uint8_t)((h >> 3) & 7u);
      for (uint32_t r = 0; r < num && r < (uint32_t)bgs::kMlSlots; ++r) o[2 + r] = (uint8_t)((h >> (6 + 3 * r)) & 7u);
      continue;
    }
    for (uint32_t r = 0; r < num && r < (uint32_t)bgs::kMlSlots; ++r) {
      const uint32_t s = (h >> (6 + 3 * r)) & 7u;
      if (s >= (uint32_t)bgs::kMlSlots) continue;
      float* m = (float*)dst + (i * bgs::kMlSlots + s) * 18;
      const uint32_t* S = w.data() + (size_t)(2 + s * bgs::kMlSlotPlanes) * n + i;
      for (int j = 0; j < 9; ++j) std::memcpy(&m[j], &S[(size_t)j * n], 4);  // bg_pattern[6], bg_intensity[3]
      const uint32_t mx = S[(size_t)11 * n], mn = S[(size_t)12 * n];
      for (int c = 0; c < 3; ++c) m[9 + c] = (float)((mx >> (8 * c)) & 0xffu), m[12 + c] = (float)((mn >> (8 * c)) & 0xffu);
      std::memcpy(&m[15], &S[(size_t)9 * n], 4), std::memcpy(&m[16], &S[(size_t)10 * n], 4);
      m[17] = (float)((w[n + i] >> (3 * s)) & 7u);
    }
  }
  return (int64_t)nb;
}

constexpr Family kMultilayer = [] {
  Family f{};
  f.check_geometry = ml_check_geometry, f.allocate = ml_allocate, f.key = ml_key, f.run = ml_run, f.get_state = ml_get_state;
  f.needs_byte_mask = always;
  return f;
}();
// frozen: the wrapper hands its values over at its first frame only (MultiLayerBGS.cpp:69-193)
constexpr ParamBlock<bgs_multilayer_params> kMultilayerBlock{&bgs_engine::ml, &kMultilayer, "bgs_multilayer_params", kMlName, ml_defaults, ml_check, false};
