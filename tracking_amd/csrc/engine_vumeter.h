// engine_vumeter.h — host side of package_bgs/av/VuMeter (BGS_VUMETER): the setters' replacement rules, model allocation, the
// per-stream schedule, the post-filter and the state export.  Included by bgs_hip.hip inside its anonymous namespace; kernel in
// kernel_vumeter.h.
//
// The wrapper (VuMeter.cpp:33-86) re-reads its XML on every frame but hands alpha, binSize and threshold to its model once, on the
// first frame; the engine does the same at bgs_create (bgs_set_params keeps them, enableFilter is live).  m_nCount is the model
// object's own counter (restarted by Init on a stream's first frame): kept per stream, so streams of different ages share a launch.

struct VuState : FamilyState {
  DevPtr<float> hist;             // histogram planes [bin][S][n]
  DevPtr<uint8_t> bg, raw, tmp;   // background bytes, the unfiltered and the eroded mask, [S][n] each
  DevPtr<uint32_t> live;          // live-bin bitmaps [S][n] (none in the dense variant)
  std::vector<int> count;         // m_nCount of each stream's model object
};
VuState& vu_of(const bgs_engine* e) { return state_of<VuState>(e); }

// TBackgroundVuMeter::SetBinSize / SetAlpha / SetThreshold (TBackgroundVuMeter.h:47-54): out-of-range values are replaced, not refused
struct VuModelParams {
  int bin_size, bin_count;
  double alpha, threshold;
};

VuModelParams vu_model_params(const bgs_params& p) {
  VuModelParams m{};
  m.bin_size = (p.vu_bin_size > 0 && p.vu_bin_size < 255) ? p.vu_bin_size : 8;
  m.alpha = (p.vu_alpha > 0.0 && p.vu_alpha < 1.0) ? p.vu_alpha : 0.995;
  m.threshold = (p.vu_threshold > 0.0 && p.vu_threshold < 1.0) ? p.vu_threshold : 0.03;
  m.bin_count = 256 / m.bin_size;
  return m;
}

// variant of kernel_vumeter.h: the bitmap holds 32 bins; more than that (binSize < 8) is the dense path
int vu_mode(const bgs_engine* e) { return vu_model_params(e->p).bin_count > bgs::kVuLiveMaxBins ? 0 : e->knob.vu_sparse; }

uint64_t vu_key(const bgs_engine*, int) { return 0; }  // first frames and the quiet phase go into the launch as per-stream bits

int vu_check_geometry(bgs_algo, int, int, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "VuMeter reads 3-channel frames only (cvCvtColor(frame, gray, CV_RGB2GRAY) asserts, VuMeter.cpp:49)");
  return BGS_OK;
}

int vu_allocate(bgs_engine* e) {
  const size_t n = e->n, S = (size_t)e->S;
  if (n * S >= (size_t)1 << 31) return fail(BGS_ERR_INVALID, "VuMeter: streams x pixels must stay below 2^31");
  const VuModelParams mp = vu_model_params(e->p);
  VuState& st = make_state<VuState>(e);
  int rc = model_allocate(e, st.hist, (size_t)mp.bin_count * S * n * sizeof(float));
  if (rc) return rc;
  DMALLOC(st.bg, S * n);
  DMALLOC(st.raw, S * n);
  DMALLOC(st.tmp, S * n);
  if (vu_mode(e)) DMALLOC(st.live, S * n * sizeof(uint32_t));
  st.count.assign(S, 0);
  // Nothing is initialised here: a stream's first frame reads neither planes nor bitmap (VuArgs::init_mask)
  return BGS_OK;
}

// One frame of VuMeter::process for streams [first, first+count).
int vu_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  VuState& st = vu_of(e);
  const size_t n = e->n;
  const VuModelParams mp = vu_model_params(e->p);
  const bool filter = e->p.vu_enable_filter != 0;
  const int mode = vu_mode(e);
  if (filter && d_bits && !d_fg) return fail(BGS_ERR_INVALID, "internal: VuMeter's filtered packed mask needs a byte mask");  // process_range provides one
  for (int f = 0; f < count; f += bgs::kVuTable) {
    const int c = std::min(bgs::kVuTable, count - f);
    const size_t o = (size_t)f * n, so = (size_t)(first + f) * n;
    bgs::VuArgs a{};
    a.cur = d_frames + o * 3;
    a.fg = filter ? ((d_fg || d_bits) ? st.raw + so : nullptr) : (d_fg ? d_fg + o : nullptr);
    a.fg_bits = (!filter && d_bits) ? d_bits + o / 64 : nullptr;
    a.bgout = d_bg ? d_bg + o : nullptr;
    a.hist = st.hist + so, a.bg = st.bg + so, a.live = st.live ? st.live + so : nullptr;
    a.plane = (size_t)e->S * n, a.npix = (uint32_t)(n * c), a.n = (uint32_t)n;
    a.bin_size = mp.bin_size, a.bin_count = mp.bin_count;
    a.alpha = (float)mp.alpha, a.inc = (float)(1.0 - mp.alpha), a.threshold = mp.threshold;
    for (int i = 0; i < c; ++i) {
      int& cnt = st.count[first + f + i];
      if (e->seen[first + f + i] == 0) cnt = 0, a.init_mask |= (uint64_t)1 << i;  // isInitOk fails -> Init(): Clear, Reset
      if (++cnt < 5) a.quiet_mask |= (uint64_t)1 << i;                            // m_nCount++ ... if(m_nCount < 5) cvSetZero(mask)
    }
    const dim3 grid(blocks_for(a.npix)), block(bgs::kBlock);
    Timed tm(e, s, mode == 0 ? "vumeter_kernel<dense>" : mode == 1 ? "vumeter_kernel<live>" : "vumeter_kernel<live,masked>");
    if (mp.bin_count == 32) {  // the default: the unrolled kernels
      if (mode == 0) hipLaunchKernelGGL((bgs::vumeter_kernel<0, 32>), grid, block, 0, s, a);
      if (mode == 1) hipLaunchKernelGGL((bgs::vumeter_kernel<1, 32>), grid, block, 0, s, a);
      if (mode == 2) hipLaunchKernelGGL((bgs::vumeter_kernel<2, 32>), grid, block, 0, s, a);
    } else {
      if (mode == 0) hipLaunchKernelGGL((bgs::vumeter_kernel<0, 0>), grid, block, 0, s, a);
      if (mode == 1) hipLaunchKernelGGL((bgs::vumeter_kernel<1, 0>), grid, block, 0, s, a);
      if (mode == 2) hipLaunchKernelGGL((bgs::vumeter_kernel<2, 0>), grid, block, 0, s, a);
    }
  }
  if (filter && d_fg) {  // cv::erode(fg, fg, cv::Mat()) then cv::medianBlur(fg, fg, 5), on every frame (the first four filter zeros)
    const size_t so = (size_t)first * n;
    bgs::MorphArgs er{st.raw + so, st.tmp + so, e->rows, e->cols, 0, 3};
    bgs::morph_launch(er, count, s);
    bgs::MorphArgs md{st.tmp + so, d_fg, e->rows, e->cols, 3, 5};
    bgs::morph_launch(md, count, s);
    if (d_bits) hipLaunchKernelGGL(bgs::mask_pack_kernel, dim3(blocks_for(n * count)), dim3(bgs::kBlock), 0, s, (const uint8_t*)d_fg, d_bits, n * count);
  }
  *flags = BGS_FG_VALID | BGS_BG_VALID;
  return BGS_OK;
}

// bgs_get_state planes (include/bgs_hip.h): "hist" in the reference's dense form whatever the variant keeps
int64_t vu_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const VuState& st = vu_of(e);
  const size_t n = e->n;
  if (!strcmp(plane, "count")) {
    const int64_t v = st.count[stream];
    return copy_host(plane, dst, cap, &v, 8);
  }
  if (!strcmp(plane, "background")) return copy_plane(plane, dst, cap, st.bg + (size_t)stream * n, n);
  if (!strcmp(plane, "hist")) {
    const size_t B = (size_t)vu_model_params(e->p).bin_count;
    if (cap < B * n * 4) return too_small(plane);
    float* o = (float*)dst;
    if (e->seen[stream] == 0) {  // Reset(): every bin 0 (the planes hold whatever the previous run of this stream left)
      memset(o, 0, B * n * 4);
      return (int64_t)(B * n * 4);
    }
    for (size_t b = 0; b < B; ++b)
      if (fetch(o + b * n, st.hist + (b * e->S + stream) * n, n * 4)) return BGS_ERR_HIP;
    if (st.live) {  // a clear bit means 0; the plane element was never written or is stale
      std::vector<uint32_t> bits(n);
      if (fetch(bits.data(), st.live + (size_t)stream * n, n * 4)) return BGS_ERR_HIP;
      for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < n; ++i)
          if (!((bits[i] >> b) & 1u)) o[b * n + i] = 0.0f;
    }
    return (int64_t)(B * n * 4);
  }
  return unknown_plane(e, plane);
}

void vu_reset_stream(bgs_engine* e, int stream) { vu_of(e).count[stream] = 0; }

// VuMeter.cpp:42-47: SetAlpha / SetBinSize / SetThreshold on the first frame only; enableFilter is live
void vu_keep_frozen(bgs_params& p, const bgs_params& old) { p.vu_bin_size = old.vu_bin_size, p.vu_alpha = old.vu_alpha, p.vu_threshold = old.vu_threshold; }

// the filtered mask is finished by erode + median: its packed form is made from the byte mask
bool vu_needs_byte_mask(const bgs_engine* e) { return e->p.vu_enable_filter != 0; }

constexpr Family kVuMeter = [] {
  Family f{};
  f.check_geometry = vu_check_geometry, f.allocate = vu_allocate, f.key = vu_key, f.run = vu_run, f.get_state = vu_get_state;
  f.reset_stream = vu_reset_stream, f.keep_frozen = vu_keep_frozen, f.needs_byte_mask = vu_needs_byte_mask, f.bg_channels = 1;
  return f;
}();
