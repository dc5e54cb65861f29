// engine_imbs.h — host side of package_bgs/db IndependentMultimodalBGS (BGS_IMBS; kernel_imbs.h); included inside bgs_hip.hip's
// anonymous namespace.
//
// The wrapper constructs BackgroundSubtractorIMBS(fps) once (IndependentMultimodalBGS.cpp:8) and the model sizes its arrays at its
// first frame: the parameters are taken when the geometry is set, and a later bgs_set_imbs_params succeeds and leaves the values in
// force.  Which frames sample, build or detect depends on the data (the gate on pixel 0, sudden_change), so the host never knows:
// every frame enqueues the same launches and the kernels read their stream's control block.  Nothing here waits for the device.

struct ImbsState : FamilyState {
  DevPtr<uint32_t> bins, model, persist, smp, bgimg;  // [S][cap][n], [S][M][n], [S][n] x 3
  DevPtr<uint8_t> lab, plane, tmp, ones, zeros;       // [S][n] each
  DevPtr<int> L1, L0, Q, A;                           // [S][n] each
  DevPtr<bgs::ImbsCtl> ctl;                           // [S]
  uint32_t cap = 0, M = 0;
};
ImbsState& imbs_of(const bgs_engine* e) { return state_of<ImbsState>(e); }

constexpr const char* kImbsName = "IndependentMultimodalBGS";

void imbs_defaults(bgs_imbs_params* p) {  // imbs.hpp:43-56, fps as IndependentMultimodalBGS.cpp:8 passes it
  std::memset(p, 0, sizeof(*p));
  p->struct_size = (uint32_t)sizeof(*p);
  p->fps = 10, p->fgThreshold = 15, p->associationThreshold = 5, p->samplingPeriod = 500, p->minBinHeight = 2, p->numSamples = 30;
  p->alpha = 0.65f, p->beta = 1.15f, p->tau_s = 60, p->tau_h = 40, p->minArea = 30, p->persistencePeriod = 10000, p->morphologicalFiltering = 0;
}

// Needs no device: checked before the GPU is opened.
int imbs_check(bgs_algo, const bgs_imbs_params& p) {
  if (!(p.fps > 0) || !std::isfinite(p.fps))
    return fail(BGS_ERR_UNSUPPORTED, "%s: fps %g must be finite and above 0 (fps 0 is wall-clock time in the reference, which cannot be reproduced)", kImbsName, p.fps);
  if (p.minBinHeight == 0) return fail(BGS_ERR_UNSUPPORTED, "%s: minBinHeight 0 (the reference divides by it in initialize before its own clamp)", kImbsName);
  if (p.numSamples < 2 || p.numSamples > BGS_IMBS_MAX_SAMPLES)
    return fail(BGS_ERR_UNSUPPORTED, "%s: numSamples %u is outside 2..%d (bin heights and counters are packed into 6 bits)", kImbsName, p.numSamples, BGS_IMBS_MAX_SAMPLES);
  if (p.numSamples / p.minBinHeight == 0)  // maxBgBins
    return fail(BGS_ERR_UNSUPPORTED, "%s: numSamples %u / minBinHeight %u leaves no model slot (maxBgBins 0)", kImbsName, p.numSamples, p.minBinHeight);
  if (p.tau_s < 0 || p.tau_s > 255 || p.tau_h < 0 || p.tau_h > 255)
    return fail(BGS_ERR_UNSUPPORTED, "%s: tau_s %d / tau_h %d must be 0..255 (uchar members)", kImbsName, p.tau_s, p.tau_h);
  if (!std::isfinite(p.alpha) || !std::isfinite(p.beta) || !std::isfinite(p.minArea))
    return fail(BGS_ERR_UNSUPPORTED, "%s: alpha, beta and minArea must be finite", kImbsName);
  return BGS_OK;
}
int imbs_check_geometry(bgs_algo, int, int, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "%s: 3-channel frames only (CV_Assert(frame.channels() == 3), imbs.cpp:169)", kImbsName);
  return BGS_OK;
}

int imbs_allocate(bgs_engine* e) {
  const bgs_imbs_params& p = e->imbs;  // the defaults or what passed imbs_check in bgs_set_imbs_params
  const size_t S = (size_t)e->S, n = e->n;
  if (S * n >= (size_t)1 << 30) return fail(BGS_ERR_INVALID, "%s: streams x pixels must stay below 2^30 (32-bit labels, areas in half pixels)", kImbsName);
  ImbsState& st = make_state<ImbsState>(e);
  st.cap = p.numSamples, st.M = p.numSamples / p.minBinHeight;  // maxBgBins, never recomputed
  int rc = model_allocate(e, st.bins, S * st.cap * n * 4);
  if (rc) return rc;
  DMALLOC(st.model, S * st.M * n * 4);
  DMALLOC(st.persist, S * n * 4);
  DMALLOC(st.smp, S * n * 4);
  DMALLOC(st.bgimg, S * n * 4);
  DMALLOC(st.lab, S * n);
  DMALLOC(st.plane, S * n);
  DMALLOC(st.tmp, S * n);
  DMALLOC(st.ones, S * n);
  DMALLOC(st.zeros, S * n);
  DMALLOC(st.L1, S * n * 4);
  DMALLOC(st.L0, S * n * 4);
  DMALLOC(st.Q, S * n * 4);
  DMALLOC(st.A, S * n * 4);
  DMALLOC(st.ctl, S * sizeof(bgs::ImbsCtl));
  // Nothing is initialised here: a stream's first frame clears its model on the launch stream (imbs_run)
  return BGS_OK;
}

// a stream's first frame clears its model; everything else is in the control block on the device
uint64_t imbs_key(const bgs_engine* e, int i) { return e->seen[i] == 0; }

bgs::ImbsArgs imbs_args(const bgs_engine* e, int first, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg) {
  const ImbsState& st = imbs_of(e);
  const bgs_imbs_params& p = e->imbs;
  const size_t f = (size_t)first, n = e->n;
  bgs::ImbsArgs a{};
  a.cur = d_frames, a.fg = d_fg, a.bgout = d_bg;
  a.bins = st.bins + f * st.cap * n, a.model = st.model + f * st.M * n, a.persist = st.persist + f * n, a.smp = st.smp + f * n, a.bgimg = st.bgimg + f * n;
  a.lab = st.lab + f * n, a.plane = st.plane + f * n, a.ones = st.ones + f * n, a.zeros = st.zeros + f * n;
  a.L1 = st.L1 + f * n, a.L0 = st.L0 + f * n, a.Q = st.Q + f * n, a.A = st.A + f * n;
  a.ctl = st.ctl + f;
  a.n = (uint32_t)n, a.cap = st.cap, a.M = st.M, a.rows = e->rows, a.cols = e->cols;
  a.fg_thr = p.fgThreshold, a.assoc = p.associationThreshold, a.min_bin = p.minBinHeight, a.persist_period = p.persistencePeriod;
  a.alpha = p.alpha, a.beta = p.beta, a.tau_s = p.tau_s, a.tau_h = p.tau_h;
  a.step = 1000. / p.fps, a.min_area = p.minArea, a.max_area = 0.6 * (unsigned)n;  // double maxArea = 0.6 * numPixels
  return a;
}

int imbs_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const ImbsState& st = imbs_of(e);
  const bgs_imbs_params& p = e->imbs;
  const size_t n = e->n, N = n * (size_t)count;
  const bgs::ImbsArgs a = imbs_args(e, first, d_frames, d_fg, d_bg);
  const dim3 block(bgs::kBlock), per(blocks_for(n), (unsigned)count), all(blocks_for(N)), lanes(((unsigned)count + 63) / 64);
  if (e->seen[first] == 0) {  // initialize(): the whole run is on its first frame (imbs_key).  isValid false, heights 0, flags 0, maps 0
    HIP_TRY(hipMemsetAsync(a.bins, 0, (size_t)count * st.cap * n * 4, s));
    HIP_TRY(hipMemsetAsync(a.model, 0, (size_t)count * st.M * n * 4, s));
    HIP_TRY(hipMemsetAsync(a.persist, 0, N * 4, s));
    HIP_TRY(hipMemsetAsync(a.smp, 0, N * 4, s));
    HIP_TRY(hipMemsetAsync(a.bgimg, 0, N * 4, s));
    hipLaunchKernelGGL(bgs::imbs_ctl_init_kernel, lanes, dim3(64), 0, s, a.ctl, count, p.numSamples, p.samplingPeriod);
  }
  {
    Timed tm(e, s, "imbs_detect_kernel");
    hipLaunchKernelGGL(bgs::imbs_detect_kernel, per, block, 0, s, a);
  }
  uint8_t* tmp = st.tmp + (size_t)first * n;
  if (p.morphologicalFiltering) {  // MORPH_OPEN then MORPH_CLOSE with a 3x3 box, morphologyEx's default border
    bgs::morph_launch(bgs::MorphArgs{a.plane, tmp, e->rows, e->cols, 0, 3}, count, s);
    bgs::morph_launch(bgs::MorphArgs{tmp, a.plane, e->rows, e->cols, 1, 3}, count, s);
    bgs::morph_launch(bgs::MorphArgs{a.plane, tmp, e->rows, e->cols, 1, 3}, count, s);
    bgs::morph_launch(bgs::MorphArgs{tmp, a.plane, e->rows, e->cols, 0, 3}, count, s);
  }
  {  // areaThresholding
    const int allRows = e->rows * count;
    hipLaunchKernelGGL(bgs::imbs_area_prep_kernel, per, block, 0, s, a, (const uint8_t*)a.plane);
    hipLaunchKernelGGL(bgs::cc_init_kernel, all, block, 0, s, (const uint8_t*)a.ones, a.L1, allRows, e->cols, e->rows, 1);
    hipLaunchKernelGGL(bgs::cc_merge_kernel, all, block, 0, s, a.L1, allRows, e->cols, e->rows, 1);
    hipLaunchKernelGGL(bgs::cc_compress_kernel, all, block, 0, s, a.L1, N);
    hipLaunchKernelGGL(bgs::cc_init_kernel, all, block, 0, s, (const uint8_t*)a.zeros, a.L0, allRows, e->cols, e->rows, 0);
    hipLaunchKernelGGL(bgs::cc_merge_kernel, all, block, 0, s, a.L0, allRows, e->cols, e->rows, 0);
    hipLaunchKernelGGL(bgs::cc_compress_kernel, all, block, 0, s, a.L0, N);
    hipLaunchKernelGGL(bgs::imbs_area_quads_kernel, per, block, 0, s, a);
    hipLaunchKernelGGL(bgs::imbs_area_push_kernel, per, block, 0, s, a);
    hipLaunchKernelGGL(bgs::imbs_area_chain_kernel, per, block, 0, s, a);
    hipLaunchKernelGGL(bgs::imbs_final_kernel, per, block, 0, s, a);
  }
  hipLaunchKernelGGL(bgs::imbs_control_kernel, lanes, dim3(64), 0, s, a, count);
  hipLaunchKernelGGL(bgs::imbs_sample_kernel, per, block, 0, s, a);
  hipLaunchKernelGGL(bgs::imbs_out_kernel, per, block, 0, s, a);
  if (d_bits) hipLaunchKernelGGL(bgs::mask_pack_kernel, dim3(blocks_for(N)), block, 0, s, (const uint8_t*)d_fg, d_bits, N);  // n % 64 == 0 here; d_fg: needs_byte_mask
  *flags = BGS_FG_VALID | BGS_BG_VALID;  // the learning phase hands out zero images, as the reference does with putText a no-op
  return BGS_OK;
}

// bgs_get_state planes (include/bgs_hip.h), unpacked
int64_t imbs_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const ImbsState& st = imbs_of(e);
  const size_t n = e->n, k = (size_t)stream;
  const bool fresh = e->seen[stream] == 0;  // initialize() has not run: what it would leave
  if (!strcmp(plane, "control")) {
    bgs::ImbsCtl c{};
    c.ns = e->imbs.numSamples, c.sp = e->imbs.samplingPeriod;
    uint32_t w0 = 0;
    if (!fresh && (fetch(&c, st.ctl + k, sizeof(c)) || fetch(&w0, st.model + k * st.M * n, 4))) return BGS_ERR_HIP;
    const double v[10] = {c.ts, c.prev_ts, (double)c.pbft, (double)c.bfc, (double)c.ns, (double)c.sp, (double)c.bg_reset, (double)c.sudden, (double)st.M, (double)((w0 & bgs::kImbsValid) != 0)};
    return copy_host(plane, dst, cap, v, sizeof(v));
  }
  if (!strcmp(plane, "persistence")) {
    if (cap < n * 4) return too_small(plane);
    if (fresh) return std::memset(dst, 0, n * 4), (int64_t)(n * 4);
    return copy_plane(plane, dst, cap, st.persist + k * n, n * 4);
  }
  const bool bins = !strcmp(plane, "bins"), model = !strcmp(plane, "model");
  if (!bins && !model) return unknown_plane(e, plane);
  const size_t slots = bins ? st.cap : st.M, rec = bins ? 5 : 6, nb = n * slots * rec;
  if (cap < nb) return too_small(plane);
  std::memset(dst, 0, nb);
  if (fresh) return (int64_t)nb;
  std::vector<uint32_t> w(n * slots);
  if (fetch(w.data(), bins ? st.bins + k * slots * n : st.model + k * slots * n, n * slots * 4)) return BGS_ERR_HIP;
  uint8_t* o = (uint8_t*)dst;
  for (size_t s = 0; s < slots; ++s)
    for (size_t i = 0; i < n; ++i) {
      const uint32_t v = w[s * n + i];
      uint8_t* r = o + (i * slots + s) * rec;
      r[0] = (uint8_t)v, r[1] = (uint8_t)(v >> 8), r[2] = (uint8_t)(v >> 16);
      if (bins) r[3] = (uint8_t)((v >> 24) & 0x3f), r[4] = (uint8_t)(v >> 31);
      else r[3] = (uint8_t)((v >> 30) & 1), r[4] = (uint8_t)(v >> 31), r[5] = (uint8_t)((v >> 24) & 0x3f);
    }
  return (int64_t)nb;
}

constexpr Family kImbs = [] {
  Family f{};
  f.check_geometry = imbs_check_geometry, f.allocate = imbs_allocate, f.key = imbs_key, f.run = imbs_run, f.get_state = imbs_get_state;
  f.needs_byte_mask = always;
  return f;
}();
// frozen: the model sizes its arrays at its first frame (initialize) and the wrapper never constructs it again
constexpr ParamBlock<bgs_imbs_params> kImbsBlock{&bgs_engine::imbs, &kImbs, "bgs_imbs_params", kImbsName, imbs_defaults, imbs_check, false};
