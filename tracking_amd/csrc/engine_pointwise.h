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

// ------------------------------------------------------------------------------ FrameDifference, WeightedMovingMean / Variance
// frame history ring (FD: 2 slots, WMM/WMV: 3): frame t of stream s lives in ring[t % nring] + s*n*ch.  The ring is the engine's
// (the generic clip and host paths use it, free_all frees it): these classes have no state of their own.
int ring_allocate(bgs_engine* e) {
  e->nring = e->algo == BGS_FRAME_DIFF ? 2 : 3;
  for (int i = 0; i < e->nring; ++i) DMALLOC(e->ring[i], e->n * e->S * e->ch);
  return BGS_OK;
}

uint64_t ring_key(const bgs_engine* e, int i) {  // ring slot + warm-up level
  return (uint64_t)(e->rpos[i] % e->nring) | (uint64_t)std::min<int64_t>(e->seen[i], e->nring - 1) << 8;
}

int ring_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const int64_t t = e->seen[first];
  const int C = e->ch;
  const size_t npix = e->n * count, off = e->n * first, fb = npix * C;
  const bool whole = (first == 0 && count == e->S);
  if (e->borrow && !whole && !e->borrow_in_clip) return fail(BGS_ERR_INVALID, "borrowed frame history needs whole-batch calls");
  bgs::FrameArgs a = frame_args(e, count, d_frames, d_fg, d_bg, d_bits);
  const int R = e->nring, warm = R - 1;
  const int64_t rp = e->rpos[first];  // the same for every stream of the run (launch_key)
  const uint8_t *cur = d_frames, *h1 = nullptr, *h2 = nullptr;
  if (e->borrow) {
    h1 = e->borrowed[0], h2 = e->borrowed[1];
  } else {
    uint8_t* slot = e->ring[rp % R] + off * C;
    if (cur != slot) HIP_TRY(hipMemcpyAsync(slot, cur, fb, hipMemcpyDeviceToDevice, s));  // keep a private copy as history
    cur = slot;
    if (t >= 1) h1 = e->ring[(rp + R - 1) % R] + off * C;
    if (t >= 2 && R == 3) h2 = e->ring[(rp + R - 2) % R] + off * C;
  }
  if (t >= warm) {
    a.cur = cur, a.p1 = h1, a.p2 = h2;
    const int G = pick_group(a, C, e->algo == BGS_FRAME_DIFF ? 16 : 4);
    if (e->algo == BGS_FRAME_DIFF)
      LAUNCH_FRAME_KERNEL(framediff_kernel, "framediff_kernel");
    else if (e->algo == BGS_WMM)
      LAUNCH_FRAME_KERNEL(wmm_kernel, "wmm_kernel");
    else
      LAUNCH_FRAME_KERNEL(wmv_kernel, "wmv_kernel");
    *flags = BGS_FG_VALID | (e->algo == BGS_WMM ? BGS_BG_VALID : 0u);
  }
  if (e->borrow) e->borrowed[1] = e->borrowed[0], e->borrowed[0] = d_frames;
  return BGS_OK;
}

int64_t ring_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t n = e->n, off = n * stream, C = (size_t)e->ch;
  const int64_t t = e->seen[stream], rp = e->rpos[stream];
  if (!strcmp(plane, "prev1") && t >= 1) return copy_plane(plane, dst, cap, e->ring[(rp + e->nring - 1) % e->nring] + off * C, n * C);
  if (!strcmp(plane, "prev2") && e->nring == 3 && t >= 2) return copy_plane(plane, dst, cap, e->ring[(rp + e->nring - 2) % e->nring] + off * C, n * C);
  return unknown_plane(e, plane);
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

// (Re)build ABL's lookup table for the current alpha on e->stream().  Called when the geometry is set and when bgs_set_params
// changes alpha; both drain the device first / the stream after, so no launch on any stream sees a half-written table.
int abl_build_lut(bgs_engine* e) {
  SbgState& st = sbg_of(e);
  if (!st.lut) HIP_TRY(hipMalloc((void**)&st.lut.p, 256 * 256));
  hipLaunchKernelGGL(bgs::abl_lut_kernel, dim3(256), dim3(bgs::kBlock), 0, e->stream(), st.lut.p, e->p.alpha, 1 - e->p.alpha);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream()));
  st.lut_alpha = e->p.alpha, st.lut_valid = true;
  return BGS_OK;
}

int sbg_allocate(bgs_engine* e) {
  SbgState& st = make_state<SbgState>(e);
  DMALLOC(st.bg, e->n * e->S * e->ch);
  return e->algo == BGS_ABL ? abl_build_lut(e) : BGS_OK;
}

uint64_t sfd_key(const bgs_engine* e, int i) { return e->seen[i] == 0; }

uint64_t abl_key(const bgs_engine* e, int i) {
  const bgs_params& p = e->p;
  return (uint64_t)(e->seen[i] == 0) | (uint64_t)(((p.limit > 0 && p.limit < e->counter[i]) || p.limit == -1) ? 2 : 0) | (uint64_t)(p.limit > 0 ? std::min<int64_t>(e->counter[i], (int64_t)p.limit + 1) : 0) << 2;
}

int sbg_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const int C = e->ch;
  const size_t npix = e->n * count, off = e->n * first, fb = npix * C;
  bgs::FrameArgs a = frame_args(e, count, d_frames, d_fg, d_bg, d_bits);
  uint8_t* st = sbg_of(e).bg + off * C;
  if (e->seen[first] == 0) HIP_TRY(hipMemcpyAsync(st, d_frames, fb, hipMemcpyDeviceToDevice, s));  // img_input.copyTo(img_background)
  a.p1 = st;
  if (e->algo == BGS_STATIC_FRAME_DIFF) {
    a.bg = nullptr;
    const int G = pick_group(a, C);
    LAUNCH_FRAME_KERNEL(framediff_kernel, "framediff_kernel");
    if (d_bg) HIP_TRY(hipMemcpyAsync(d_bg, st, fb, hipMemcpyDeviceToDevice, s));
  } else {
    a.state_out = st;
    a.alpha = p.alpha, a.beta = 1 - p.alpha;
    const int64_t cnt = e->counter[first];
    a.update = ((p.limit > 0 && p.limit < cnt) || p.limit == -1) ? 1 : 0;
    const int G = pick_group(a, C, 4);  // 4 pixels per lane: 42 VGPRs -> two 1024-lane workgroups per CU (16: 128 VGPRs, one); measured 0.126 vs 0.134 ms
    {
      Timed t__(e, s, "abl_kernel");
      const size_t per_tile = (size_t)bgs::kAblBlock * G, ntiles = (npix + per_tile - 1) / per_tile;
      // persistent: exactly as many workgroups as are resident at once (1 or 2 per CU, by registers), each walking its share of the tiles
      const dim3 block(bgs::kAblBlock);
#define ABL_CASE(GV, CV, UV)                                                                                                               \
  if (G == GV && C == CV && (a.update != 0) == UV) {                                                                                       \
    /* resident workgroups per CU of this instantiation: a property of the code object (the library is gfx950-only), cached per   \
       process; atomic because engines may be driven from several host threads */                                                  \
    static std::atomic<int> per_cu_cache{0};                                                                                               \
    int per_cu = per_cu_cache.load(std::memory_order_relaxed);                                                                             \
    if (!per_cu) {                                                                                                                         \
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bgs::abl_kernel<GV, CV, UV>, bgs::kAblBlock, 0) != hipSuccess || per_cu < 1) per_cu = 1; \
      per_cu_cache.store(per_cu, std::memory_order_relaxed);                                                                               \
    }                                                                                                                                      \
    const dim3 grid((unsigned)std::min<size_t>(ntiles, (size_t)per_cu * e->n_cu));                                                        \
    hipLaunchKernelGGL((bgs::abl_kernel<GV, CV, UV>), grid, block, 0, s, a, (const uint8_t*)sbg_of(e).lut.p);                                   \
  }
      ABL_CASE(16, 3, true) ABL_CASE(4, 3, true) ABL_CASE(1, 3, true) ABL_CASE(16, 1, true) ABL_CASE(4, 1, true) ABL_CASE(1, 1, true)
      ABL_CASE(16, 3, false) ABL_CASE(4, 3, false) ABL_CASE(1, 3, false) ABL_CASE(16, 1, false) ABL_CASE(4, 1, false) ABL_CASE(1, 1, false)
#undef ABL_CASE
    }
    if (a.update && p.limit > 0 && p.limit < cnt)
      for (int i = first; i < first + count; ++i) e->counter[i]++;
  }
  *flags = BGS_FG_VALID | BGS_BG_VALID;
  return BGS_OK;
}

int64_t sbg_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t nb = e->n * e->ch;
  if (!strcmp(plane, "bg")) return copy_plane(plane, dst, cap, sbg_of(e).bg + nb * stream, nb);
  return unknown_plane(e, plane);
}

int abl_apply_params(bgs_engine* e) {
  if (sbg_of(e).lut_valid && e->p.alpha == sbg_of(e).lut_alpha) return BGS_OK;
  // a launch still in flight on some stream may be reading the table: let the device drain before it is rewritten
  if (hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(BGS_ERR_HIP, "device sync failed");
  return abl_build_lut(e);
}

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
  if (e->seen[first] == 0) {  // SigmaDeltaBGS.cpp:33-39: allocate + initialise, return without output
    HIP_TRY(hipMemcpyAsync(mt, d_frames, fb, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(bgs::sigmadelta_init_vt_kernel, dim3(blocks_for(fb)), dim3(bgs::kBlock), 0, s, vt, fb, e->cols, (int)(uint8_t)p.sd_min_var);
    return BGS_OK;
  }
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
  if (e->seen[stream] >= 1 && !strcmp(plane, "vt")) return copy_plane(plane, dst, cap, st.vt + nb * stream, nb);
  if ((e->seen[stream] >= 1 && !strcmp(plane, "mt")) || !strcmp(plane, "bg")) return copy_plane(plane, dst, cap, st.mt + nb * stream, nb);  // "bg": Mt under the name of the other byte classes
  return unknown_plane(e, plane);
}

constexpr Family kSigmaDelta = [] {
  Family f{};
  f.check_geometry = sd_check_geometry, f.allocate = sd_allocate, f.key = sfd_key, f.run = sd_run, f.get_state = sd_get_state;
  return f;
}();
