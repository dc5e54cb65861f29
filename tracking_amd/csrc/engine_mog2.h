// engine_mog2.h — host side of MixtureOfGaussianV2BGS (BGS_MOG2; kernel_mog2.h: tiles of ranked weights + fixed-slot records +
// rank->slot meta words): the automatic choice of how a launch loads the model, the per-frame and the clip launch, the state export.
// Included by bgs_hip.hip inside its anonymous namespace, after engine_mog1.h (mog_lr_key, mog_clip_fusable).

int mog2_check(bgs_algo, const bgs_params& p) {
  if (p.mog2_nmixtures != bgs::kMog2K) return fail(BGS_ERR_UNSUPPORTED, "MOG2 kernel is built for K=%d mixtures, got %d", bgs::kMog2K, p.mog2_nmixtures);
  return BGS_OK;
}

int mog2_check_geometry(bgs_algo, int, int, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "MixtureOfGaussianV2BGS needs 3 channels: getBackgroundImage asserts nchannels == 3 (MixtureOfGaussianV2BGS.cpp:59)");
  return BGS_OK;
}

// Automatic choice of how a per-frame launch loads a pixel's model (kernel_mog2.h; results are identical, only speed differs):
//   1 eager   everything at once, no dependent loads: right when most pixels have most modes and need them;
//   2 count   only the modes a pixel has (one dependent round): quiet scenes, one or two modes per pixel;
//   4 filter  summaries first, then only the records they cannot rule out (one dependent round, +4 B per mode for the
//             summaries): pays when at least half of a pixel's records are ruled out (modes far apart).
// About 256 sampled workgroups of a sampling filter-kernel launch count, per pixel, the modes it has and the records that kernel loads
// or would load.  When another kernel is current, every 16th launch - every 4th of a stream's first 64 - is a filter launch for
// that purpose (a launch that delivers the shadow test or the background image samples in the count kernel instead).  While the
// filter kernel is current every launch samples until two polls in a row have confirmed it, then every 8th: a sample costs a copy, a
// memset and an event record on the launch stream between two update kernels.  The host never blocks: the counters come back through a pinned buffer and an event that is queried before
// every launch; it switches at once on clear evidence, else when two samples in a row ask for the same other mode.
struct Mog2State : FamilyState {
  DevPtr<uint8_t> model;     // tiles of ranked weights + fixed-slot records + rank->slot meta words (kernel_mog2.h)
  int sparse_now = 2;        // what auto mode currently runs
  int sparse_want = 2;       // what the last poll asked for (a switch needs two polls in a row)
  unsigned launches = 0;     // auto mode: per-frame launches so far (every 16th one samples)
  // while the filter kernel is current: a sampling launch is followed by a copy, a memset and an event record on the launch stream.
  // Once two polls in a row have confirmed mode 4 only every 8th filter launch samples; a poll that asks for another mode brings
  // back a sample on each of the next 8 launches.
  unsigned confirmed4 = 0;       // polls in a row that found mode 4 current and asked for it
  unsigned every_left = 0;       // filter launches that still sample each time
  unsigned filter_launches = 0;  // filter launches in the steady state (every 8th one samples)
  DevPtr<unsigned> d_stat;   // device: {record slots sampled, modes live, records needed after the summaries}
  // pinned copies of the counters, a ring of kStatSlots posts (one per sampling launch, each with its event): a host that runs far
  // ahead of the device still finds the most recent sample that has COMPLETED when it looks
  static constexpr int kStatSlots = 8;
  unsigned* h_stat = nullptr;  // [kStatSlots][3]
  hipEvent_t stat_ev[kStatSlots] = {nullptr};
  bool stat_posted[kStatSlots] = {false};
  unsigned stat_seq = 0;  // posts so far
  ~Mog2State() override {
    model.reset(), d_stat.reset();
    if (h_stat) (void)hipHostFree(h_stat);
    for (hipEvent_t ev : stat_ev)
      if (ev) (void)hipEventDestroy(ev);
  }
};
Mog2State& mog2_of(const bgs_engine* e) { return state_of<Mog2State>(e); }

void mog2_stat_read(Mog2State& st) {
  // the newest post whose copy has completed; everything older is dropped with it
  int slot = -1;
  for (unsigned back = 1; back <= (unsigned)Mog2State::kStatSlots && back <= st.stat_seq; ++back) {
    const int i = (int)((st.stat_seq - back) % Mog2State::kStatSlots);
    if (!st.stat_posted[i]) break;  // already consumed (and so is everything older)
    if (slot < 0 && hipEventQuery(st.stat_ev[i]) == hipSuccess) slot = i;
    if (slot >= 0) st.stat_posted[i] = false;
  }
  if (slot < 0) return;
  const unsigned* hs = st.h_stat + 3 * slot;
  const unsigned total = hs[0], live = hs[1], need = hs[2];
  if (total < 64 * 5) return;
  const float lf = (float)live / (float)total, nf = (float)need / (float)total;
  const int want = (nf < 0.5f * lf && lf - nf > 0.1f) ? 4 : lf < 0.7f ? 2 : 1;
  const bool clear = (want == 4 && nf < 0.35f * lf) || (want != 4 && st.sparse_now == 4 && nf > 0.8f * lf);
  static const bool debug = getenv("BGS_DEBUG_STAT") != nullptr;
  if (debug)
    fprintf(stderr, "[bgs] mog2 auto: %u record slots sampled, %.3f live, %.3f needed after the summaries -> mode %d (now %d)\n", total, lf, nf, want, st.sparse_now);
  const bool confirms = want == 4 && st.sparse_now == 4;  // (the poll that switches to mode 4 does not count)
  if (want != st.sparse_now && (clear || want == st.sparse_want)) st.sparse_now = want;
  st.sparse_want = want;
  if (confirms) {
    st.confirmed4++;
  } else {
    st.confirmed4 = 0;
    st.every_left = 8;
  }
}
void mog2_stat_post(Mog2State& st, hipStream_t s) {
  const int i = (int)(st.stat_seq % Mog2State::kStatSlots);  // the oldest slot is reused (its event re-recorded) if nobody read it
  (void)hipMemcpyAsync(st.h_stat + 3 * i, st.d_stat, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, s);
  (void)hipMemsetAsync(st.d_stat, 0, 3 * sizeof(unsigned), s);
  (void)hipEventRecord(st.stat_ev[i], s);
  st.stat_posted[i] = true;
  st.stat_seq++;
}

int launch_mog2(bgs_engine* e, bgs::Mog2Args& a, hipStream_t s, bool timed = true) {
  const bgs_params& p = e->p;
  // shadow test only when it can change the delivered mask: not thresholded, or the threshold separates shadow from foreground
  a.shadow = p.mog2_detect_shadows && (!p.enable_threshold || ((p.mog2_shadow_value > p.threshold) != (255 > p.threshold)));
  a.want_bg = a.bgimg != nullptr, a.packed = a.fg_bits != nullptr;
  a.xcd_swizzle = e->knob.xcd_swizzle, a.complete = e->knob.mog2_complete;
  Mog2State& st = mog2_of(e);
  const bool autom = timed && e->knob.mog2_sparse == 3;
  if (autom) mog2_stat_read(st);
  int mode = e->knob.mog2_sparse == 3 ? st.sparse_now : e->knob.mog2_sparse;
  const bool every_mean = a.shadow || a.want_bg;  // shadow test and background image read every mode's mean: nothing to rule out,
  if (mode >= 4 && every_mean) mode = 2;          // and the filter kernel is built without them (kernel_mog2.h, FEAT)
  // auto mode: the filter kernel's sampled workgroups count what each way of loading would read; when another kernel is current,
  // every 16th launch (every 4th of the first 64) goes through the filter kernel anyway so that the choice keeps following the scene.
  // A launch that reads every mean samples in the count kernel instead, which posts the same three numbers the filter kernel would
  // with nothing ruled out.
  bool sample = false;
  if (autom && mode != 4) {
    const unsigned n = st.launches++;
    if ((n & (n < 64 ? 3u : 15u)) == 0) sample = true, mode = every_mean ? 2 : 4;
  } else if (autom) {
    // the filter kernel is current: every launch samples until two polls in a row have confirmed it, then every 8th
    if (st.every_left > 0 || st.confirmed4 < 2) {
      sample = true;
      if (st.every_left > 0) st.every_left--;
    } else {
      sample = (st.filter_launches++ & 7u) == 0;
    }
  }
  if (mode >= 4 && every_mean) return fail(BGS_ERR_INVALID, "MOG2: the filter kernel cannot deliver the shadow test or the background image");
  a.sparse = mode;
  a.stat = sample ? st.d_stat.p : nullptr;
  if (a.packed && a.npix % 64) return fail(BGS_ERR_UNSUPPORTED, "packed mask needs pixels %% 64 == 0");
  Timed t(e, s, "mog2_update_kernel", timed);
  const dim3 grid(blocks_for(a.npix)), block(bgs::kBlock);  // one pixel per lane (round 2's 1 / 2 / 4 comparison: equal or better everywhere)
  unsigned every = 1;  // sample about 256 workgroups per launch whatever the grid: enough to decide, few enough atomics not to show
  while (grid.x / every > 256) every <<= 1;
  a.stat_mask = every - 1;
  // (occupancy, DESIGN.md 6.1: 2 / 3 / 4 / 5 waves per SIMD 2.15 / 1.50 / 1.22 / 1.09 ms - profiles/r04_mog2_occupancy_ab.txt; the
  // 60-VGPR filter kernel at 5 / 6 / 7 / 8 waves: 6 is fastest by about 1 %, which is what it is held to - profiles/mog2_stream_ab.txt)
  if (mode >= 4)
    hipLaunchKernelGGL((bgs::mog2_update_kernel<bgs::kMog2Filter>), grid, block, 0, s, a);
  else if (mode >= 2)
    hipLaunchKernelGGL((bgs::mog2_update_kernel<bgs::kMog2Count>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((bgs::mog2_update_kernel<bgs::kMog2Eager>), grid, block, 0, s, a);
  if (a.stat) mog2_stat_post(st, s);
  return BGS_OK;
}

void mog2_fill_args(const bgs_engine* e, bgs::Mog2Args& m, double lr) {
  const bgs_params& p = e->p;
  m.state = mog2_of(e).model;
  m.alphaT = (float)lr, m.alpha1 = 1.f - m.alphaT, m.prune = (float)(-lr * (double)p.mog2_ct);
  m.Tb = p.mog2_var_threshold, m.TB = p.mog2_background_ratio, m.Tg = p.mog2_var_threshold_gen;
  m.s_min = bgs::mog2_smin(bgs::mog2_tq(m.Tb > m.Tg ? m.Tb : m.Tg));  // the summaries' rejection rule, as one bound on the bucket distance (kernel_mog2.h)
  m.varInit = p.mog2_var_init, m.varMin = p.mog2_var_min, m.varMax = p.mog2_var_max, m.tau = p.mog2_tau;
  m.thr = p.threshold, m.enable_thr = p.enable_threshold, m.shadow_val = p.mog2_shadow_value;
}

void mog2_clear(bgs_engine* e, const bgs::Mog2Args& m, hipStream_t s) {
  hipLaunchKernelGGL(bgs::mog2_clear_kernel, dim3(blocks_for(m.npix)), dim3(bgs::kBlock), 0, s, m);
}

// One launch over `fuse` (2, 4 or 8) consecutive frames of streams whose model starts at c.m.state_off (kernel_mog2.h, clip launches)
int launch_mog2_clip(bgs_engine* e, bgs::Mog2ClipArgs& c, int fuse, hipStream_t s) {
  const bgs_params& p = e->p;
  bgs::Mog2Args& a = c.m;
  a.shadow = p.mog2_detect_shadows && (!p.enable_threshold || ((p.mog2_shadow_value > p.threshold) != (255 > p.threshold)));
  a.want_bg = a.bgimg != nullptr, a.packed = a.fg_bits != nullptr;
  a.xcd_swizzle = e->knob.xcd_swizzle, a.complete = e->knob.mog2_complete;
  a.sparse = e->knob.mog2_sparse == 0 ? 0 : 1;  // clip launches load every record at once (kernel_mog2.h)
  a.stat = nullptr;
  if (a.packed && a.npix % 64) return fail(BGS_ERR_UNSUPPORTED, "packed mask needs pixels %% 64 == 0");
  Timed t(e, s, "mog2_clip_kernel");
  const dim3 grid(blocks_for(a.npix)), block(bgs::kBlock);
  unsigned every = 1;
  while (grid.x / every > 256) every <<= 1;
  a.stat_mask = every - 1;
#define MOG2_CLIP_CASE(TV) \
  if (fuse == TV) hipLaunchKernelGGL((bgs::mog2_clip_kernel<TV>), grid, block, 0, s, c);
  MOG2_CLIP_CASE(2) MOG2_CLIP_CASE(4) MOG2_CLIP_CASE(8)
#undef MOG2_CLIP_CASE
  return BGS_OK;
}

size_t mog2_state_bytes(const bgs_engine* e) {
  const size_t P = e->n * e->S;
  return (P + bgs::kMog2Tile - 1) / bgs::kMog2Tile * bgs::kMog2TileBytes;
}

int mog2_allocate(bgs_engine* e) {
  Mog2State& st = make_state<Mog2State>(e);
  HIP_TRY(hipMalloc((void**)&st.d_stat.p, 3 * sizeof(unsigned)));
  HIP_TRY(hipMemsetAsync(st.d_stat, 0, 3 * sizeof(unsigned), e->stream()));  // ordered: allocate() drains e->stream() before it returns
  HIP_TRY(hipHostMalloc((void**)&st.h_stat, 3 * Mog2State::kStatSlots * sizeof(unsigned), hipHostMallocDefault));
  for (hipEvent_t& ev : st.stat_ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  return model_allocate(e, st.model, mog2_state_bytes(e));
}

uint64_t mog2_key(const bgs_engine* e, int i) { return mog_lr_key(e, i, e->p.mog2_history, 2); }

int mog2_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  double lr = p.alpha;
  int64_t nframes = e->seen[first];
  bgs::Mog2Args m{};
  m.state_off = e->n * first, m.npix = e->n * count;
  mog2_fill_args(e, m, 0.0);
  if (nframes == 0 || lr >= 1) {  // needToInitialize: bgmodel = zeros, modesUsed = 0
    mog2_clear(e, m, s);
    nframes = 0;
  }
  ++nframes;
  const int64_t n2 = 2 * nframes;
  lr = (lr >= 0 && nframes > 1) ? lr : 1. / (double)std::min<int64_t>(n2, p.mog2_history);
  mog2_fill_args(e, m, lr);
  m.frame = d_frames, m.fg = d_fg, m.bgimg = d_bg, m.fg_bits = d_bits;
  int rc = launch_mog2(e, m, s);
  if (rc) return rc;
  if (nframes == 1)  // re-initialisation restarts the count (the streams of a run may otherwise have different ages: launch_key)
    for (int i = first; i < first + count; ++i) e->seen[i] = 0;
  *flags = BGS_FG_VALID | BGS_BG_VALID;
  return BGS_OK;
}

int mog2_clip_fused(bgs_engine* e, int first, int count, int fuse, size_t slab, const uint8_t* fr, uint8_t* fg, uint8_t* bg, uint64_t* bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const int64_t seen = e->seen[first];
  bgs::Mog2ClipArgs c{};
  c.m.state_off = e->n * first, c.m.npix = e->n * count;
  mog2_fill_args(e, c.m, 0.0);
  if (seen == 0) mog2_clear(e, c.m, s);  // needToInitialize on a stream's first frame
  for (int j = 0; j < fuse; ++j) {       // the learning rate of each frame, as the single-frame path computes it
    const int64_t nf = seen + j + 1;
    const double lr = (p.alpha >= 0 && nf > 1) ? p.alpha : 1. / (double)std::min<int64_t>(2 * nf, p.mog2_history);
    c.alphaT[j] = (float)lr, c.alpha1[j] = 1.f - c.alphaT[j], c.prune[j] = (float)(-lr * (double)p.mog2_ct);
  }
  c.m.frame = fr, c.m.fg = fg, c.m.bgimg = bg, c.m.fg_bits = bits;
  c.frame_stride = slab * 3, c.fg_stride = slab, c.bg_stride = slab * 3, c.bits_stride = slab / 64;
  *flags = BGS_FG_VALID | BGS_BG_VALID;
  return launch_mog2_clip(e, c, fuse, s);
}

// canonical export: "w" [K][n], "var" [K][n], "mu" [K][3][n] floats, "nmodes" [n] bytes — whatever the device layout
int64_t mog2_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t n = e->n, off = n * stream;
  int p0 = -1, np = 0;
  if (!strcmp(plane, "w")) p0 = 0, np = 5;
  if (!strcmp(plane, "var")) p0 = 5, np = 5;
  if (!strcmp(plane, "mu")) p0 = 10, np = 15;
  if (!strcmp(plane, "summary")) p0 = 100, np = 5;  // uint32 [K][n] by rank: the 16-bit word q0 | q1 << 5 | q2 << 10 | class << 15 (kernel_mog2.h; for the invariant test)
  const bool nm = !strcmp(plane, "nmodes") || !strcmp(plane, "summary_valid");  // bytes [n]; summary_valid: bit 15 of the meta word
  const bool want_valid = !strcmp(plane, "summary_valid");
  if (p0 < 0 && !nm) return unknown_plane(e, plane);
  // device layout (kernel_mog2.h): weights by rank, {var, mean} records in fixed slots, meta = rank -> slot.  Exported in the
  // reference's array order (rank); entries past a pixel's mode count are zero, as in the reference's zero-initialised bgmodel.
  const size_t need = nm ? n : (size_t)np * n * 4;
  if (cap < need) return too_small(plane);
  const size_t T = bgs::kMog2Tile, TB = bgs::kMog2TileBytes;
  const size_t t0 = off / T, t1 = (off + n + T - 1) / T;
  std::vector<uint8_t> tiles((t1 - t0) * TB);
  if (fetch(tiles.data(), mog2_of(e).model + t0 * TB, tiles.size())) return BGS_ERR_HIP;
  for (size_t i = 0; i < n; ++i) {
    const size_t sp = off + i, in = sp % T;
    const uint8_t* tb = tiles.data() + (sp / T - t0) * TB;
    const float* w = reinterpret_cast<const float*>(tb) + in;
    const float* rec = reinterpret_cast<const float*>(tb + bgs::kMog2RecOff) + in * 4;
    const uint16_t* sum = reinterpret_cast<const uint16_t*>(tb + bgs::kMog2SumOff) + in;
    const unsigned meta = reinterpret_cast<const uint16_t*>(tb + bgs::kMog2MetaOff)[in];
    if (nm) {
      ((uint8_t*)dst)[i] = want_valid ? (uint8_t)((meta >> 15) & 1u) : (uint8_t)bgs::mog2_meta_count(meta);
      continue;
    }
    for (int r = 0; r < bgs::kMog2K; ++r) {
      const unsigned f = (meta >> (3 * r)) & 7u;
      const float* rc = f ? rec + (size_t)(f - 1) * T * 4 : nullptr;
      if (p0 == 100) ((uint32_t*)dst)[(size_t)r * n + i] = f ? sum[(size_t)(f - 1) * T] : 0u;
      if (p0 == 0) ((float*)dst)[(size_t)r * n + i] = f ? w[(size_t)r * T] : 0.f;
      if (p0 == 5) ((float*)dst)[(size_t)r * n + i] = f ? rc[0] : 0.f;
      if (p0 == 10)
        for (int c = 0; c < 3; ++c) ((float*)dst)[((size_t)r * 3 + c) * n + i] = f ? rc[1 + c] : 0.f;
    }
  }
  return (int64_t)need;
}

constexpr Family kMog2 = [] {
  Family f{};
  f.check = mog2_check, f.check_geometry = mog2_check_geometry, f.allocate = mog2_allocate, f.key = mog2_key, f.run = mog2_run;
  f.get_state = mog2_get_state, f.clip_fused = mog2_clip_fused, f.clip_fusable = mog_clip_fusable;
  return f;
}();
