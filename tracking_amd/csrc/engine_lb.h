// engine_lb.h — host side of the five package_bgs/lb/ classes (BGS_LB_*): checks, the 0..255 -> double parameter mapping, model
// allocation, the per-stream schedule and the state export.  Included by bgs_hip.hip inside its anonymous namespace; kernels in
// kernel_lb.h.
//
// The wrappers (LB*.cpp:31-74) re-read their XML and call setBGModelParameter(id, 0..255) on every frame, after InitModel on the
// first one: Init() therefore sees the constructor's m_noise (50), and every Update() - the first included - the XML's values.
// The SOMs' training counter m_K is the model object's own state (restarted by Init, advanced by Update while m_K <= m_TSteps, and
// m_TSteps may change between frames), so it is kept per stream here and not derived from bgs_engine::seen.

struct LbState : FamilyState {
  DevPtr<double> model;  // planar doubles [S][P][n]
  DevPtr<int32_t> k;     // MoG: modes per pixel [S][n]
  DevPtr<uint8_t> bg;    // the SOMs' background bytes [S][n*3]
  std::vector<int> mk;   // the SOMs' training counter m_K, one per stream
};
LbState& lb_of(const bgs_engine* e) { return state_of<LbState>(e); }

bool is_lb_som(bgs_algo a) { return a == BGS_LB_ADAPTIVE_SOM || a == BGS_LB_FUZZY_ADAPTIVE_SOM; }

const char* lb_name(bgs_algo a) {
  switch (a) {
    case BGS_LB_SIMPLE_GAUSSIAN: return "LBSimpleGaussian";
    case BGS_LB_FUZZY_GAUSSIAN: return "LBFuzzyGaussian";
    case BGS_LB_MOG: return "LBMixtureOfGaussians";
    case BGS_LB_ADAPTIVE_SOM: return "LBAdaptiveSOM";
    default: return "LBFuzzyAdaptiveSOM";
  }
}

int lb_planes_of(bgs_algo a) { return is_lb_som(a) ? bgs::kLbSomPlanes : a == BGS_LB_MOG ? bgs::kLbMogPlanes : bgs::kLbGaussPlanes; }

// What the reference leaves undefined or order-dependent is refused.
int lb_check(bgs_algo algo, const bgs_params& p) {
  const char* nm = lb_name(algo);
  const struct { const char* key; int v; } all[] = {{"sensitivity", p.lb_sensitivity}, {"bgThreshold", p.lb_bg_threshold}, {"learningRate", p.lb_learning_rate},
      {"noiseVariance", p.lb_noise_variance}, {"trainingSensitivity", p.lb_training_sensitivity}, {"trainingLearningRate", p.lb_training_learning_rate},
      {"trainingSteps", p.lb_training_steps}};
  for (const auto& f : all)
    if (f.v < 0 || f.v > 255) return fail(BGS_ERR_UNSUPPORTED, "%s %s must be 0..255 (setBGModelParameter's range), got %d", nm, f.key, f.v);
  if (!is_lb_som(algo) && p.lb_noise_variance == 0) return fail(BGS_ERR_UNSUPPORTED, "%s noiseVariance 0: the variances reach 0 and the Mahalanobis distance divides by them", nm);
  if (algo == BGS_LB_MOG && p.lb_bg_threshold == 255)
    return fail(BGS_ERR_UNSUPPORTED, "%s bgThreshold 255: m_T = 1 may never be exceeded and the reference then reads kBG uninitialised (BGModelMog.cpp:146)", nm);
  if (is_lb_som(algo) && p.lb_training_steps == 0) return fail(BGS_ERR_UNSUPPORTED, "%s trainingSteps 0: alpha is 0 / 0 at m_K = 0 (BGModelSom.cpp:194)", nm);
  return BGS_OK;
}

// setBGModelParameter of the five models, in double and in the reference's order of operations
struct LbModelParams {
  double threshold, noise, alpha, bg_threshold;            // Gaussians, MoG
  double eps1, eps2, alpha1, alpha2;                       // SOMs
  int tsteps;
};

LbModelParams lb_model_params(bgs_algo algo, const bgs_params& p) {
  auto dv = [](int v) { return (double)v / 255.0; };
  LbModelParams m{};
  double d = dv(p.lb_sensitivity);
  m.threshold = 100.0 * d * d;
  m.eps2 = 255.0 * 255.0 * d * d * d * d;
  d = dv(p.lb_training_sensitivity);
  m.eps1 = 255.0 * 255.0 * d * d * d * d;
  d = dv(p.lb_noise_variance);
  m.noise = 100.0 * d;
  d = dv(p.lb_learning_rate);
  m.alpha = d * d * d;
  const double wmax = 4.0;  // the largest entry of the 3 x 3 Pascal kernel (BGModelSom.cpp:77-99)
  m.alpha2 = d * d * d / wmax;
  d = dv(p.lb_training_learning_rate);
  m.alpha1 = d * d * d / wmax;
  m.bg_threshold = dv(p.lb_bg_threshold);
  d = dv(p.lb_training_steps);
  m.tsteps = (int)(255.0 * d);
  (void)algo;
  return m;
}

uint64_t lb_key(const bgs_engine* e, int i) { return e->seen[i] == 0; }

int lb_allocate(bgs_engine* e) {
  if (e->ch != 3) return fail(BGS_ERR_UNSUPPORTED, "%s reads 3-channel frames only (BGModel::InitModel copies into an 8UC3 image, lb/BGModel.cpp:72)", lb_name(e->algo));
  const size_t n = e->n, S = (size_t)e->S;
  if (n * S >= (size_t)1 << 31) return fail(BGS_ERR_INVALID, "lb: streams x pixels must stay below 2^31");
  LbState& st = make_state<LbState>(e);
  int rc = model_allocate(e, st.model, S * n * lb_planes_of(e->algo) * sizeof(double));
  if (rc) return rc;
  if (e->algo == BGS_LB_MOG) DMALLOC(st.k, S * n * sizeof(int32_t));
  if (is_lb_som(e->algo)) DMALLOC(st.bg, S * n * 3);
  st.mk.assign(S, 0);
  // Nothing is initialised here: a stream's first frame builds its model inside the launch (LbArgs::init)
  return BGS_OK;
}

// Kernel arguments of streams [f, f + c) of a run that starts at stream `first`: the parameters of this call and the pointers of
// one frame (d_* point at the run's first stream).  `init`: the frame is these streams' first one.
bgs::LbArgs lb_args(const bgs_engine* e, const LbModelParams& mp, bool init, int first, int f, int c, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits) {
  const LbState& st = lb_of(e);
  const size_t n = e->n, o = (size_t)(f - first) * n;
  bgs::LbArgs a{};
  a.n = (uint32_t)n, a.init = init;
  a.threshold = mp.threshold, a.noise = mp.noise, a.noise0 = 50.0, a.alpha = mp.alpha, a.bg_threshold = mp.bg_threshold;
  a.cur = d_frames + o * 3, a.fg = d_fg ? d_fg + o : nullptr, a.bg = d_bg ? d_bg + o * 3 : nullptr;
  a.fg_bits = d_bits ? d_bits + o / 64 : nullptr;
  a.model = st.model + (size_t)f * lb_planes_of(e->algo) * n;
  a.k = st.k ? st.k + (size_t)f * n : nullptr, a.bgplane = st.bg ? st.bg + (size_t)f * n * 3 : nullptr;
  a.npix = (uint32_t)(n * c);
  a.bps = (uint32_t)blocks_for(n);
  return a;
}

// BGModelSom::Update's phase test for one frame of one stream: calibration while m_K <= m_TSteps (frame 1 counts), alpha with the
// integers promoted to double.  Advances the stream's counter.
void lb_som_schedule(const LbModelParams& mp, int& mk, double* alpha, double* eps) {
  if (mk <= mp.tsteps) {
    *eps = mp.eps1, *alpha = mp.alpha1 - (double)mk * (mp.alpha1 - mp.alpha2) / (double)mp.tsteps;
    ++mk;
  } else {
    *eps = mp.eps2, *alpha = mp.alpha2;
  }
}

// the two Gaussian kernels take two pixels per lane when asked to and n is even: pairs of pixels never straddle two streams then,
// and every double2 is aligned
bool lb_two_px(const bgs_engine* e) { return e->knob.lb_px == 2 && e->n % 2 == 0; }

// One frame for streams [first, first+count), `init`: their first one.
int lb_frame(bgs_engine* e, bool init, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s) {
  LbState& st = lb_of(e);
  const LbModelParams mp = lb_model_params(e->algo, e->p);
  if (!is_lb_som(e->algo)) {
    const bgs::LbArgs a = lb_args(e, mp, init, first, first, count, d_frames, d_fg, d_bg, d_bits);
    const size_t npix = a.npix;
    if (e->algo == BGS_LB_MOG) {
      Timed tm(e, s, "lb_mog_kernel");
      hipLaunchKernelGGL(bgs::lb_mog_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, a);
    } else {
      const bool fuzzy = e->algo == BGS_LB_FUZZY_GAUSSIAN;
      Timed tm(e, s, fuzzy ? "lb_fuzzy_gauss_kernel" : "lb_gauss_kernel");
      if (lb_two_px(e)) {
        if (fuzzy)
          hipLaunchKernelGGL((bgs::lb_gauss_kernel<true, 2>), dim3(blocks_for(npix / 2)), dim3(bgs::kBlock), 0, s, a);
        else
          hipLaunchKernelGGL((bgs::lb_gauss_kernel<false, 2>), dim3(blocks_for(npix / 2)), dim3(bgs::kBlock), 0, s, a);
      } else {
        if (fuzzy)
          hipLaunchKernelGGL((bgs::lb_gauss_kernel<true, 1>), dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, a);
        else
          hipLaunchKernelGGL((bgs::lb_gauss_kernel<false, 1>), dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, a);
      }
    }
  } else {
    // Streams whose counters differ get their own table entry in the same launch.
    std::vector<double> al(count), ep(count);
    bool same = true;
    for (int i = 0; i < count; ++i) {
      int& mk = st.mk[first + i];
      if (init) mk = 0;
      lb_som_schedule(mp, mk, &al[i], &ep[i]);
      same = same && al[i] == al[0] && ep[i] == ep[0];
    }
    const bool fuzzy = e->algo == BGS_LB_FUZZY_ADAPTIVE_SOM;
    for (int f = 0; f < count; f += same ? count : bgs::kLbTable) {
      const int c = same ? count : std::min(bgs::kLbTable, count - f);
      bgs::LbArgs a = lb_args(e, mp, init, first, first + f, c, d_frames, d_fg, d_bg, d_bits);
      a.uniform = same;
      const dim3 grid(a.bps * (unsigned)c);
      for (int i = 0; i < (same ? 1 : c); ++i) a.alpha_s[i] = al[f + i], a.eps_s[i] = ep[f + i];
      Timed tm(e, s, fuzzy ? "lb_fuzzy_som_kernel" : "lb_som_kernel");
      if (fuzzy)
        hipLaunchKernelGGL(bgs::lb_som_kernel<true>, grid, dim3(bgs::kBlock), 0, s, a);
      else
        hipLaunchKernelGGL(bgs::lb_som_kernel<false>, grid, dim3(bgs::kBlock), 0, s, a);
    }
  }
  return BGS_OK;
}

// One frame of LB*::process for streams [first, first+count), which share lb_key.
int lb_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  *flags = BGS_FG_VALID | BGS_BG_VALID;
  return lb_frame(e, e->seen[first] == 0, first, count, d_frames, d_fg, d_bg, d_bits, s);
}

template <int T>
void lb_launch_clip(const bgs_engine* e, hipStream_t s, const bgs::LbClipArgs& c) {
  const dim3 block(bgs::kBlock);
  const size_t npix = c.a.npix;
  switch (e->algo) {
    case BGS_LB_MOG: hipLaunchKernelGGL((bgs::lb_mog_clip_kernel<T>), dim3(blocks_for(npix)), block, 0, s, c); break;
    case BGS_LB_ADAPTIVE_SOM: hipLaunchKernelGGL((bgs::lb_som_clip_kernel<false, T>), dim3(c.a.bps * (unsigned)(npix / c.a.n)), block, 0, s, c); break;
    case BGS_LB_FUZZY_ADAPTIVE_SOM: hipLaunchKernelGGL((bgs::lb_som_clip_kernel<true, T>), dim3(c.a.bps * (unsigned)(npix / c.a.n)), block, 0, s, c); break;
    case BGS_LB_FUZZY_GAUSSIAN:
      if (lb_two_px(e))
        hipLaunchKernelGGL((bgs::lb_gauss_clip_kernel<true, 2, T>), dim3(blocks_for(npix / 2)), block, 0, s, c);
      else
        hipLaunchKernelGGL((bgs::lb_gauss_clip_kernel<true, 1, T>), dim3(blocks_for(npix)), block, 0, s, c);
      break;
    default:
      if (lb_two_px(e))
        hipLaunchKernelGGL((bgs::lb_gauss_clip_kernel<false, 2, T>), dim3(blocks_for(npix / 2)), block, 0, s, c);
      else
        hipLaunchKernelGGL((bgs::lb_gauss_clip_kernel<false, 1, T>), dim3(blocks_for(npix)), block, 0, s, c);
  }
}

const char* lb_clip_kernel_name(bgs_algo a) {
  switch (a) {
    case BGS_LB_SIMPLE_GAUSSIAN: return "lb_gauss_clip_kernel";
    case BGS_LB_FUZZY_GAUSSIAN: return "lb_fuzzy_gauss_clip_kernel";
    case BGS_LB_MOG: return "lb_mog_clip_kernel";
    case BGS_LB_ADAPTIVE_SOM: return "lb_som_clip_kernel";
    default: return "lb_fuzzy_som_clip_kernel";
  }
}

// `fuse` = 8 / 4 / 2 consecutive frames of streams [first, first+count) in one launch (kernel_lb.h: lb_*_clip_kernel); the streams
// have seen the same number of frames (process_clip_run).  slab: pixels from one frame of the clip to the next.
int lb_clip_fused(bgs_engine* e, int first, int count, int fuse, size_t slab, const uint8_t* fr, uint8_t* fg, uint8_t* bg, uint64_t* bits, hipStream_t s, uint32_t* flags) {
  LbState& st = lb_of(e);
  const LbModelParams mp = lb_model_params(e->algo, e->p);
  const bool init = e->seen[first] == 0;
  *flags = BGS_FG_VALID | BGS_BG_VALID;
  bgs::LbClipArgs c{};
  c.a = lb_args(e, mp, init, first, first, count, fr, fg, bg, bits);
  c.frame_stride = slab * 3, c.fg_stride = slab, c.bits_stride = slab / 64;
  if (is_lb_som(e->algo)) {
    // The training schedule of the run's frames, counter advanced per frame as lb_frame does.  Streams of one age share m_K unless
    // trainingSteps changed between calls that fed them separately: such a run takes the per-frame launches and their table.
    std::vector<int> mk(count);
    bool same = true;
    for (int i = 0; i < count; ++i) {
      mk[i] = init ? 0 : st.mk[first + i];
      for (int t = 0; t < fuse; ++t) {
        double al, ep;
        lb_som_schedule(mp, mk[i], &al, &ep);
        if (i == 0) c.alpha_t[t] = al, c.eps_t[t] = ep;
        same = same && al == c.alpha_t[t] && ep == c.eps_t[t];
      }
    }
    if (!same) {
      for (int t = 0; t < fuse; ++t) {
        int rc = lb_frame(e, init && t == 0, first, count, fr + (size_t)t * c.frame_stride, fg ? fg + (size_t)t * c.fg_stride : nullptr,
                          bg ? bg + (size_t)t * c.frame_stride : nullptr, bits ? bits + (size_t)t * c.bits_stride : nullptr, s);
        if (rc) return rc;
      }
      return BGS_OK;
    }
    for (int i = 0; i < count; ++i) st.mk[first + i] = mk[i];
  }
  Timed tm(e, s, lb_clip_kernel_name(e->algo));
  switch (fuse) {
    case 8: lb_launch_clip<8>(e, s, c); break;
    case 4: lb_launch_clip<4>(e, s, c); break;
    case 2: lb_launch_clip<2>(e, s, c); break;
    default: return fail(BGS_ERR_INVALID, "internal: lb clip run of %d frames", fuse);
  }
  return BGS_OK;
}

// bgs_get_state planes (include/bgs_hip.h), in the reference's memory order.
int64_t lb_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const LbState& st = lb_of(e);
  const size_t n = e->n;
  const int P = lb_planes_of(e->algo);
  const bool som = is_lb_som(e->algo), mog = e->algo == BGS_LB_MOG, gauss = !som && !mog;
  if (som && !strcmp(plane, "count")) {
    const int64_t v = st.mk[stream];
    return copy_host(plane, dst, cap, &v, 8);
  }
  if (som && !strcmp(plane, "bg")) return copy_plane(plane, dst, cap, st.bg + (size_t)stream * n * 3, n * 3);
  if (mog && !strcmp(plane, "k")) return copy_plane(plane, dst, cap, st.k + (size_t)stream * n, n * 4);
  // the planes made from the model: doubles per pixel of the export
  const bool mu = !strcmp(plane, "mu"), var = !strcmp(plane, "var"), w = !strcmp(plane, "w"), key = !strcmp(plane, "sortkey");
  const size_t per = som ? (!strcmp(plane, "som") ? 27 : 0) : (mu || var) ? (mog ? 9 : 3) : (mog && (w || key)) ? 3 : 0;
  if (!per) return unknown_plane(e, plane);
  if (cap < n * per * 8) return too_small(plane);
  std::vector<int32_t> K(mog ? n : 0);
  if (mog && fetch(K.data(), st.k + (size_t)stream * n, n * 4)) return BGS_ERR_HIP;
  std::vector<double> m((size_t)P * n);
  if (fetch(m.data(), st.model + (size_t)stream * P * n, m.size() * 8)) return BGS_ERR_HIP;
  double* o = (double*)dst;
  auto at = [&](int k, int f, size_t i) { return k < K[i] ? m[(size_t)(7 * k + f) * n + i] : 0.0; };  // MoG slots >= K: the constructor's zeros
  for (size_t i = 0; i < n; ++i) {
    if (som)
      for (int j = 0; j < 27; ++j) o[i * 27 + j] = m[(size_t)j * n + i];
    else if (gauss)
      for (int c = 0; c < 3; ++c) o[i * 3 + c] = m[(size_t)((mu ? 0 : 3) + c) * n + i];
    else if (mu || var)
      for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) o[(i * 3 + k) * 3 + c] = at(k, (mu ? 1 : 4) + c, i);
    else
      for (int k = 0; k < 3; ++k) {
        double v = at(k, 0, i);
        if (key && k < K[i]) v = v / std::sqrt(at(k, 6, i) + at(k, 5, i) + at(k, 4, i));  // Red + Green + Blue
        o[i * 3 + k] = v;
      }
  }
  return (int64_t)(n * per * 8);
}

void lb_reset_stream(bgs_engine* e, int stream) { lb_of(e).mk[stream] = 0; }

constexpr Family kLb = [] {
  Family f{};
  f.check = lb_check, f.allocate = lb_allocate, f.key = lb_key, f.run = lb_run, f.get_state = lb_get_state, f.reset_stream = lb_reset_stream;
  f.clip_fused = lb_clip_fused;
  return f;
}();
