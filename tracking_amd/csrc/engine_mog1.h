// engine_mog1.h — host side of MixtureOfGaussianV1BGS (BGS_MOG1; kernel_mog1.h, tiled model).  Included by bgs_hip.hip inside its
// anonymous namespace.

int mog1_check(bgs_algo, const bgs_params& p) {
  if (p.mog1_nmixtures != bgs::kMog1K) return fail(BGS_ERR_UNSUPPORTED, "MOG1 kernel is built for K=%d mixtures, got %d", bgs::kMog1K, p.mog1_nmixtures);
  return BGS_OK;
}

struct Mog1State : FamilyState {
  DevPtr<float> model;  // tiles of kMog1Tile pixels (kernel_mog1.h)
};
Mog1State& mog1_of(const bgs_engine* e) { return state_of<Mog1State>(e); }

int mog1_allocate(bgs_engine* e) {
  const size_t tile_floats = e->ch == 3 ? bgs::mog1_tile_floats<3>() : bgs::mog1_tile_floats<1>();
  const size_t tiles = (e->n * e->S + bgs::kMog1Tile - 1) / bgs::kMog1Tile;
  return model_allocate(e, make_state<Mog1State>(e).model, tiles * tile_floats * sizeof(float));
}

// MOG1 / MOG2: needToInitialize + the learning rate of stream i's next frame
uint64_t mog_lr_key(const bgs_engine* e, int i, int64_t cap, int64_t mult) {
  const double alpha = e->p.alpha;
  if (e->seen[i] == 0 || alpha >= 1) return 1;
  if (alpha >= 0) return 2;
  return 3 + (uint64_t)std::min<int64_t>(mult * (e->seen[i] + 1), cap);
}
uint64_t mog1_key(const bgs_engine* e, int i) { return mog_lr_key(e, i, e->p.mog1_history, 1); }

// lr >= 1 re-initialises the model on every frame (needToInitialize): nothing to keep in registers across the frames of a clip
bool mog_clip_fusable(const bgs_engine* e) { return e->p.alpha < 1; }

void mog1_fill_args(const bgs_engine* e, bgs::Mog1Args& m, double lr) {
  const bgs_params& p = e->p;
  const int C = e->ch;
  const double defaultNoiseSigma = 30 * 0.5;
  m.alpha = (float)lr, m.T = (float)p.mog1_background_ratio, m.vT = (float)p.mog1_var_threshold;
  m.w0 = (float)0.05;
  m.sk0 = C == 3 ? (float)(m.w0 / (defaultNoiseSigma * 2 * std::sqrt(3.))) : (float)(m.w0 / (defaultNoiseSigma * 2));
  m.var0 = (float)(defaultNoiseSigma * defaultNoiseSigma * 4);
  m.minVar = (float)(p.mog1_noise_sigma * p.mog1_noise_sigma);
  m.thr = p.threshold, m.enable_thr = p.enable_threshold, m.packed = m.fg_bits != nullptr, m.xcd_swizzle = e->knob.xcd_swizzle;
}

void mog1_clear(bgs_engine* e, const bgs::Mog1Args& m, hipStream_t s) {  // needToInitialize: bgmodel = zeros
  if (e->ch == 3)
    hipLaunchKernelGGL((bgs::mog1_clear_kernel<3>), dim3(blocks_for(m.npix)), dim3(bgs::kBlock), 0, s, m);
  else
    hipLaunchKernelGGL((bgs::mog1_clear_kernel<1>), dim3(blocks_for(m.npix)), dim3(bgs::kBlock), 0, s, m);
}

int mog1_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t*, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const int C = e->ch;
  const size_t npix = e->n * count;
  double lr = p.alpha;
  int64_t nframes = e->seen[first];
  bgs::Mog1Args m{};
  m.state = mog1_of(e).model, m.state_off = e->n * first, m.npix = npix;
  if (nframes == 0 || lr >= 1) {
    mog1_clear(e, m, s);
    nframes = 0;
  }
  ++nframes;
  lr = (lr >= 0 && nframes > 1) ? lr : 1. / (double)std::min<int64_t>(nframes, p.mog1_history);
  m.frame = d_frames, m.fg = d_fg, m.fg_bits = d_bits;
  mog1_fill_args(e, m, lr);
  {
    Timed tm(e, s, "mog1_update_kernel");
    const dim3 grid(blocks_for(npix)), block(bgs::kBlock);
    if (C == 3) hipLaunchKernelGGL((bgs::mog1_update_kernel<3>), grid, block, 0, s, m);
    if (C == 1) hipLaunchKernelGGL((bgs::mog1_update_kernel<1>), grid, block, 0, s, m);
  }
  if (nframes == 1)  // re-initialisation restarts the count (the streams of a run may otherwise have different ages: launch_key)
    for (int i = first; i < first + count; ++i) e->seen[i] = 0;
  *flags = BGS_FG_VALID;  // BackgroundSubtractorMOG has no getBackgroundImage (MixtureOfGaussianV1BGS.cpp:53)
  return BGS_OK;
}

// One launch over `fuse` (2, 4 or 8) consecutive frames, the model in registers (kernel_mog1.h); slab: pixels from one frame to the next
int mog1_clip_fused(bgs_engine* e, int first, int count, int fuse, size_t slab, const uint8_t* fr, uint8_t* fg, uint8_t*, uint64_t* bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const size_t npix = e->n * count, C = (size_t)e->ch;
  const int64_t seen = e->seen[first];
  bgs::Mog1ClipArgs c{};
  c.m.state = mog1_of(e).model, c.m.state_off = e->n * first, c.m.npix = npix;
  if (seen == 0) mog1_clear(e, c.m, s);  // needToInitialize on a stream's first frame
  c.m.frame = fr, c.m.fg = fg, c.m.fg_bits = bits;
  mog1_fill_args(e, c.m, 0.0);
  for (int j = 0; j < fuse; ++j) {
    const int64_t nf = seen + j + 1;
    c.alpha[j] = (float)((p.alpha >= 0 && nf > 1) ? p.alpha : 1. / (double)std::min<int64_t>(nf, p.mog1_history));
  }
  c.frame_stride = slab * C, c.fg_stride = slab, c.bits_stride = slab / 64;
  {
    Timed tm(e, s, "mog1_clip_kernel");
    const dim3 grid(blocks_for(npix)), block(bgs::kBlock);
#define MOG1_CLIP_CASE(CV, TV) \
  if (C == CV && fuse == TV) hipLaunchKernelGGL((bgs::mog1_clip_kernel<CV, TV>), grid, block, 0, s, c);
    MOG1_CLIP_CASE(3, 2) MOG1_CLIP_CASE(3, 4) MOG1_CLIP_CASE(3, 8) MOG1_CLIP_CASE(1, 2) MOG1_CLIP_CASE(1, 4) MOG1_CLIP_CASE(1, 8)
#undef MOG1_CLIP_CASE
  }
  *flags = BGS_FG_VALID;
  return BGS_OK;
}

// exported in the reference's order: [rank][channel][pixel] (kernel_mog1.h keeps records by slot)
int64_t mog1_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t n = e->n, off = n * stream;
  const int C = e->ch, K = bgs::kMog1K;
  int kind = -1, nf = 0;
  if (!strcmp(plane, "sortkey")) kind = 0, nf = 1;
  if (!strcmp(plane, "w")) kind = 1, nf = 1;
  if (!strcmp(plane, "mu")) kind = 2, nf = C;
  if (!strcmp(plane, "var")) kind = 3, nf = C;
  if (kind < 0) return unknown_plane(e, plane);
  const size_t need = (size_t)K * nf * n * 4;
  if (cap < need) return too_small(plane);
  const size_t T = bgs::kMog1Tile, TF = C == 3 ? bgs::mog1_tile_floats<3>() : bgs::mog1_tile_floats<1>(), t0 = off / T, t1 = (off + n + T - 1) / T;
  std::vector<float> tiles((t1 - t0) * TF);
  if (fetch(tiles.data(), mog1_of(e).model + t0 * TF, tiles.size() * 4)) return BGS_ERR_HIP;
  for (size_t i = 0; i < n; ++i) {
    const size_t sp = off + i, l = sp % T;
    const float* tb = tiles.data() + (sp / T - t0) * TF;
    const unsigned meta = reinterpret_cast<const uint16_t*>(tb + 2 * K * T + K * T * 2 * C)[l];
    for (int k = 0; k < K; ++k) {
      const int slot = (int)((meta >> (3 * k)) & 7u) - 1;  // -1: this rank never held a mode (all zeros in the reference)
      for (int c = 0; c < nf; ++c) {
        float v;
        if (kind <= 1)
          v = tb[(size_t)(kind * K + k) * T + l];
        else
          v = slot < 0 ? 0.f : tb[2 * K * T + (size_t)slot * T * 2 * C + l * 2 * C + (kind == 3 ? C : 0) + c];
        ((float*)dst)[((size_t)k * nf + c) * n + i] = v;
      }
    }
  }
  return (int64_t)need;
}

constexpr Family kMog1 = [] {
  Family f{};
  f.check = mog1_check, f.allocate = mog1_allocate, f.key = mog1_key, f.run = mog1_run, f.get_state = mog1_get_state;
  f.clip_fused = mog1_clip_fused, f.clip_fusable = mog_clip_fusable;
  return f;
}();
