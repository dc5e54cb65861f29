// engine_pointwise.h — host side of the byte-stream classes (kernel_pointwise.h): FrameDifference / WeightedMovingMean /
// WeightedMovingVariance with their frame history ring, StaticFrameDifference / AdaptiveBackgroundLearning with their background image,
// SigmaDelta.  Included by bgs_hip.hip inside its anonymous namespace; each class plugs in through its Family at the end.

#define LAUNCH_FRAME_KERNEL(KERNEL, name)                                                             \
  do {                                                                                                \
    Timed t__(e, s, name);                                                                            \
    if (C == 3) {                                                                                     \
      if (G == 16)                                                                                    \
        hipLaunchKernelGGL((bgs::KERNEL<16, 3>), dim3(blocks_for(a.npix / 16)), dim3(bgs::kBlock), 0, s, a); \
      else if (G == 4)                                                                                \
        hipLaunchKernelGGL((bgs::KERNEL<4, 3>), dim3(blocks_for(a.npix / 4)), dim3(bgs::kBlock), 0, s, a);   \
      else                                                                                            \
        hipLaunchKernelGGL((bgs::KERNEL<1, 3>), dim3(blocks_for(a.npix)), dim3(bgs::kBlock), 0, s, a);       \
    } else {                                                                                          \
      if (G == 16)                                                                                    \
        hipLaunchKernelGGL((bgs::KERNEL<16, 1>), dim3(blocks_for(a.npix / 16)), dim3(bgs::kBlock), 0, s, a); \
      else if (G == 4)                                                                                \
        hipLaunchKernelGGL((bgs::KERNEL<4, 1>), dim3(blocks_for(a.npix / 4)), dim3(bgs::kBlock), 0, s, a);   \
      else                                                                                            \
        hipLaunchKernelGGL((bgs::KERNEL<1, 1>), dim3(blocks_for(a.npix)), dim3(bgs::kBlock), 0, s, a);       \
    }                                                                                                 \
  } while (0)

// widest pixel group every pointer and the pixel count allow
// (`cap`: measured optimum of the kernel: wmm / wmv run ~10 % faster with 4 pixels per lane than with 16, abl the other way round)
int pick_group(const bgs::FrameArgs& a, int C, int cap = 16) {
  const void* ptrs[] = {a.cur, a.p1, a.p2, a.state_out, a.fg, a.bg};
  int G = 16;
  if (a.npix % 16) G = (a.npix % 4) ? 1 : 4;
  if (G > cap) G = cap;
  for (const void* p : ptrs) {
    if (!p) continue;
    if (G == 16 && !aligned(p, 16)) G = 4;
    if (G == 4 && !aligned(p, 4)) G = 1;
  }
  if (const char* env = getenv("BGS_FRAME_GROUP")) {
    const int want = atoi(env);
    if ((want == 1 || want == 4 || want == 16) && want <= G) G = want;
  }
  (void)C;
  return G;
}

// what every launch of a FrameArgs kernel starts from
bgs::FrameArgs frame_args(const bgs_engine* e, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits) {
  const bgs_params& p = e->p;
  bgs::FrameArgs a{};
  a.cur = d_frames, a.fg = d_fg, a.bg = d_bg, a.fg_bits = d_bits, a.npix = e->n * count;
  a.thr = p.threshold, a.enable_thr = p.enable_threshold, a.enable_weight = p.enable_weight;
  // The XCD-aware block order pays where a workgroup's working set is a multi-plane tile (MOG2, MOG1, dp); the byte-stream
  // kernels run 2-5 % faster in plain block order (tools/ab_pointwise.py), so they only use it at level 2 (for A/B runs).
  a.xcd_swizzle = e->knob.xcd_swizzle >= 2;
  return a;
}

// The grid of a persistent kernel of kAblBlock lanes: exactly as many workgroups as are resident at once (1 or 2 per CU, by registers),
// each walking its share of the `ntiles` tiles.  Resident workgroups per CU of an instantiation: a property of the code object (the
// library is gfx950-only), asked once per process; atomic because engines and groups may be driven from several host threads.
template <auto Kernel>
dim3 resident_grid(size_t ntiles, int n_cu) {
  static std::atomic<int> per_cu_cache{0};
  int per_cu = per_cu_cache.load(std::memory_order_relaxed);
  if (!per_cu) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, bgs::kAblBlock, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    per_cu_cache.store(per_cu, std::memory_order_relaxed);
  }
  return dim3((unsigned)std::min<size_t>(ntiles, (size_t)per_cu * n_cu));
}

// ------------------------------------------------------------------------------ FrameDifference, WeightedMovingMean / Variance
// These classes have no state of their own: their frames are in the engine's frame history ring (e->hist; FD: 2 slots, WMM / WMV: 3),
// which the generic clip and host paths drive and free_all frees.
int ring_allocate(bgs_engine* e) {
  e->hist.nring = e->algo == BGS_FRAME_DIFF ? 2 : 3;
  for (int i = 0; i < e->hist.nring; ++i) DMALLOC(e->hist.slot[i], e->n * e->S * e->ch);
  return BGS_OK;
}

uint64_t ring_key(const bgs_engine* e, int i) {  // ring slot + warm-up level
  return (uint64_t)(e->rpos[i] % e->hist.nring) | (uint64_t)std::min<int64_t>(e->seen[i], e->hist.nring - 1) << 8;
}

int ring_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const int64_t t = e->seen[first];
  const int C = e->ch;
  if (e->hist.lockstep_only() && (first != 0 || count != e->S)) return fail(BGS_ERR_INVALID, "borrowed frame history needs whole-batch calls");
  bgs::FrameArgs a = frame_args(e, count, d_frames, d_fg, d_bg, d_bits);
  FrameHistory::Frames f;  // rpos: the same for every stream of the run (launch_key)
  HIP_TRY(e->hist.resolve(e->rpos[first], t, e->n * first * C, a.npix * C, d_frames, s, &f));
  if (t >= e->hist.nring - 1) {
    a.cur = f.cur, a.p1 = f.h1, a.p2 = f.h2;
    const int G = pick_group(a, C, e->algo == BGS_FRAME_DIFF ? 16 : 4);
    if (e->algo == BGS_FRAME_DIFF)
      LAUNCH_FRAME_KERNEL(framediff_kernel, "framediff_kernel");
    else if (e->algo == BGS_WMM)
      LAUNCH_FRAME_KERNEL(wmm_kernel, "wmm_kernel");
    else
      LAUNCH_FRAME_KERNEL(wmv_kernel, "wmv_kernel");
    *flags = BGS_FG_VALID | (e->algo == BGS_WMM ? BGS_BG_VALID : 0u);
  }
  return BGS_OK;
}

int64_t ring_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t nb = e->n * e->ch;
  const uint8_t* src = e->hist.plane(e->rpos[stream], e->seen[stream], plane, nb * stream);
  return src ? copy_plane(plane, dst, cap, src, nb) : unknown_plane(e, plane);
}

constexpr Family kFrameHistory = [] {
  Family f{};
  f.allocate = ring_allocate, f.key = ring_key, f.run = ring_run, f.get_state = ring_get_state;
  return f;
}();

// ------------------------------------------------------------------------ StaticFrameDifference, AdaptiveBackgroundLearning
// State: the background image [S][n*ch]; ABL: the 256 x 256 table of background bytes for one alpha (kernel_pointwise.h)
struct SbgState : FamilyState {
  DevPtr<uint8_t> bg, lut;
  double lut_alpha = 0;  // the alpha `lut` was built for
  bool lut_valid = false;
};
SbgState& sbg_of(const bgs_engine* e) { return state_of<SbgState>(e); }

// The functions below take the state and the few scalars they need: an engine's own, or those of a group's fused class (engine_group.h).
// ABL's lookup table for `alpha`, built on the owner's stream `s` unless it is the one `st.lut` holds.  A launch still in flight on
// some stream may be reading a valid table: the device drains before it is rewritten, and `s` after, so no launch sees it half-written.
int abl_table(SbgState& st, double alpha, int device, hipStream_t s) {
  if (st.lut_valid && alpha == st.lut_alpha) return BGS_OK;
  if (st.lut_valid && (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) return fail(BGS_ERR_HIP, "device sync failed");
  if (!st.lut) HIP_TRY(hipMalloc((void**)&st.lut.p, 256 * 256));
  hipLaunchKernelGGL(bgs::abl_lut_kernel, dim3(256), dim3(bgs::kBlock), 0, s, st.lut.p, alpha, 1 - alpha);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  st.lut_alpha = alpha, st.lut_valid = true;
  return BGS_OK;
}

// AdaptiveBackgroundLearning.cpp: the background learns always (limit -1) or while the counter is past a positive limit, and only
// such a frame counts
bool abl_counts(const bgs_params& p, int64_t counter) { return p.limit > 0 && p.limit < counter; }
bool abl_updates(const bgs_params& p, int64_t counter) { return abl_counts(p, counter) || p.limit == -1; }
void abl_count(const bgs_params& p, int64_t& counter) { counter += abl_counts(p, counter); }

// a stream's first frame becomes the background image at byte `off` (img_input.copyTo(img_background))
hipError_t sbg_first_frame(SbgState& st, int64_t seen, size_t off, const uint8_t* d_frames, size_t bytes, hipStream_t s) {
  return seen ? hipSuccess : hipMemcpyAsync(st.bg + off, d_frames, bytes, hipMemcpyDeviceToDevice, s);
}

// plane `plane` of stream `stream` (nb bytes each), null for a name the class does not answer
const uint8_t* sbg_plane(const SbgState& st, int64_t, size_t nb, int stream, const char* plane) { return !strcmp(plane, "bg") ? st.bg + nb * stream : nullptr; }

int sbg_allocate(bgs_engine* e) {
  SbgState& st = make_state<SbgState>(e);
  DMALLOC(st.bg, e->n * e->S * e->ch);
  return e->algo == BGS_ABL ? abl_table(st, e->p.alpha, e->device, e->stream()) : BGS_OK;
}

uint64_t sfd_key(const bgs_engine* e, int i) { return e->seen[i] == 0; }

uint64_t abl_key(const bgs_engine* e, int i) {
  const bgs_params& p = e->p;
  return (uint64_t)(e->seen[i] == 0) | (uint64_t)(abl_updates(p, e->counter[i]) ? 2 : 0) | (uint64_t)(p.limit > 0 ? std::min<int64_t>(e->counter[i], (int64_t)p.limit + 1) : 0) << 2;
}

int sbg_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const int C = e->ch;
  const size_t npix = e->n * count, fb = npix * C;
  bgs::FrameArgs a = frame_args(e, count, d_frames, d_fg, d_bg, d_bits);
  uint8_t* st = sbg_of(e).bg + e->n * first * C;
  HIP_TRY(sbg_first_frame(sbg_of(e), e->seen[first], e->n * first * C, d_frames, fb, s));
  a.p1 = st;
  if (e->algo == BGS_STATIC_FRAME_DIFF) {
    a.bg = nullptr;
    const int G = pick_group(a, C);
    LAUNCH_FRAME_KERNEL(framediff_kernel, "framediff_kernel");
    if (d_bg) HIP_TRY(hipMemcpyAsync(d_bg, st, fb, hipMemcpyDeviceToDevice, s));
  } else {
    a.state_out = st;
    a.alpha = p.alpha, a.beta = 1 - p.alpha;
    a.update = abl_updates(p, e->counter[first]);  // the same for every stream of the run (abl_key)
    const int G = pick_group(a, C, 4);  // 4 pixels per lane: 42 VGPRs -> two 1024-lane workgroups per CU (16: 128 VGPRs, one); measured 0.126 vs 0.134 ms
    {
      Timed t__(e, s, "abl_kernel");
      const size_t per_tile = (size_t)bgs::kAblBlock * G, ntiles = (npix + per_tile - 1) / per_tile;
#define ABL_CASE(GV, CV, UV)                               \
  if (G == GV && C == CV && (a.update != 0) == UV)         \
    hipLaunchKernelGGL((bgs::abl_kernel<GV, CV, UV>), (resident_grid<bgs::abl_kernel<GV, CV, UV>>(ntiles, e->n_cu)), dim3(bgs::kAblBlock), 0, s, a, (const uint8_t*)sbg_of(e).lut.p);
      ABL_CASE(16, 3, true) ABL_CASE(4, 3, true) ABL_CASE(1, 3, true) ABL_CASE(16, 1, true) ABL_CASE(4, 1, true) ABL_CASE(1, 1, true)
      ABL_CASE(16, 3, false) ABL_CASE(4, 3, false) ABL_CASE(1, 3, false) ABL_CASE(16, 1, false) ABL_CASE(4, 1, false) ABL_CASE(1, 1, false)
#undef ABL_CASE
    }
    for (int i = first; i < first + count; ++i) abl_count(p, e->counter[i]);
  }
  *flags = BGS_FG_VALID | BGS_BG_VALID;
  return BGS_OK;
}

int64_t sbg_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t nb = e->n * e->ch;
  const uint8_t* src = sbg_plane(sbg_of(e), e->seen[stream], nb, stream, plane);
  return src ? copy_plane(plane, dst, cap, src, nb) : unknown_plane(e, plane);
}

int abl_apply_params(bgs_engine* e) { return abl_table(sbg_of(e), e->p.alpha, e->device, e->stream()); }

constexpr Family kStaticFrameDiff = [] {
  Family f{};
  f.allocate = sbg_allocate, f.key = sfd_key, f.run = sbg_run, f.get_state = sbg_get_state;
  return f;
}();

constexpr Family kAbl = [] {
  Family f = kStaticFrameDiff;
  f.key = abl_key, f.apply_params = abl_apply_params;
  return f;
}();

// ------------------------------------------------------------------------------------------------------------ SigmaDelta
int sd_check_geometry(bgs_algo, int, int, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "SigmaDeltaBGS is 3-channel only (sdLaMa091AllocInit_8u_C3R, SigmaDeltaBGS.cpp:35)");
  return BGS_OK;
}

struct SdState : FamilyState {
  DevPtr<uint8_t> mt, vt;  // sdLaMa091's Mt and Vt images [S][n*3]
};
SdState& sd_of(const bgs_engine* e) { return state_of<SdState>(e); }

// SigmaDeltaBGS.cpp:33-39: a stream's first frame allocates and initialises (Mt = the frame, Vt = the minimum) and returns without output
int sd_first_frame(SdState& st, size_t off, const uint8_t* d_frames, size_t bytes, int cols, const bgs_params& p, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(st.mt + off, d_frames, bytes, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(bgs::sigmadelta_init_vt_kernel, dim3(blocks_for(bytes)), dim3(bgs::kBlock), 0, s, st.vt + off, bytes, cols, (int)(uint8_t)p.sd_min_var);
  return BGS_OK;
}

// plane `mt` / `vt` of stream `stream` (nb bytes each) once the stream has seen a frame, null before and for every other name
const uint8_t* sd_plane(const SdState& st, int64_t seen, size_t nb, int stream, const char* plane) {
  return seen < 1 ? nullptr : !strcmp(plane, "mt") ? st.mt + nb * stream : !strcmp(plane, "vt") ? st.vt + nb * stream : nullptr;
}

int sd_allocate(bgs_engine* e) {
  SdState& st = make_state<SdState>(e);
  DMALLOC(st.mt, e->n * e->S * 3);
  DMALLOC(st.vt, e->n * e->S * 3);
  return BGS_OK;
}

int sd_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t*, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const size_t npix = e->n * count, off = e->n * first, fb = npix * 3;
  uint8_t *mt = sd_of(e).mt + off * 3, *vt = sd_of(e).vt + off * 3;
  if (e->seen[first] == 0) return sd_first_frame(sd_of(e), off * 3, d_frames, fb, e->cols, p, s);
  bgs::SigmaDeltaArgs q{};
  q.cur = d_frames, q.mt = mt, q.vt = vt, q.fg = d_fg, q.fg_bits = d_bits, q.npix = npix;
  q.N = (uint32_t)p.sd_amp_factor, q.vmin = (uint8_t)p.sd_min_var, q.vmax = (uint8_t)p.sd_max_var, q.xcd_swizzle = e->knob.xcd_swizzle >= 2;
  int G = 16;
  if (npix % 16 || !aligned(d_frames, 16) || !aligned(mt, 16) || !aligned(vt, 16) || (d_fg && !aligned(d_fg, 16))) G = (npix % 4 || !aligned(d_frames, 4) || !aligned(mt, 4) || (d_fg && !aligned(d_fg, 4))) ? 1 : 4;
  {
    Timed tm(e, s, "sigmadelta_kernel");
    if (G == 16) hipLaunchKernelGGL((bgs::sigmadelta_kernel<16>), dim3(blocks_for(npix / 16)), dim3(bgs::kBlock), 0, s, q);
    if (G == 4) hipLaunchKernelGGL((bgs::sigmadelta_kernel<4>), dim3(blocks_for(npix / 4)), dim3(bgs::kBlock), 0, s, q);
    if (G == 1) hipLaunchKernelGGL((bgs::sigmadelta_kernel<1>), dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, q);
  }
  *flags = BGS_FG_VALID;
  return BGS_OK;
}

int64_t sd_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t nb = e->n * 3;
  const SdState& st = sd_of(e);
  // "bg": Mt under the name of the other byte classes, at any age (an engine's answer; a fused SigmaDelta has no such plane)
  const uint8_t* src = !strcmp(plane, "bg") ? st.mt + nb * stream : sd_plane(st, e->seen[stream], nb, stream, plane);
  return src ? copy_plane(plane, dst, cap, src, nb) : unknown_plane(e, plane);
}

constexpr Family kSigmaDelta = [] {
  Family f{};
  f.check_geometry = sd_check_geometry, f.allocate = sd_allocate, f.key = sfd_key, f.run = sd_run, f.get_state = sd_get_state;
  return f;
}();
