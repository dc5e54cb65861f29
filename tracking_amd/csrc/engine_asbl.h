// engine_asbl.h — host side of AdaptiveSelectiveBackgroundLearning (BGS_ASBL; kernels in kernel_stencil.h, the gray kernel and its
// launch macro in kernel_pointwise.h / engine_pointwise.h).  Included by bgs_hip.hip inside its anonymous namespace.

// a ping-pong pair of gray backgrounds [S][n] (the 3x3 median reads neighbours' OLD background), which of them is current per stream,
// and the two tables of kAsblLutRows rows (learning then detection phase) with the alphas they were built for
struct AsblState : FamilyState {
  DevPtr<uint8_t> bg[2], lut;
  std::vector<uint8_t> flip;
  double lut_alpha[2] = {0, 0};
  bool lut_valid = false;
};
AsblState& asbl_of(const bgs_engine* e) { return state_of<AsblState>(e); }

// ASBL's two tables (learning / detection phase), same rules as abl_build_lut
int asbl_build_lut(bgs_engine* e) {
  AsblState& st = asbl_of(e);
  const size_t one = (size_t)bgs::kAsblLutRows * 256;
  if (!st.lut) HIP_TRY(hipMalloc((void**)&st.lut.p, 2 * one));
  const bgs_params& p = e->p;
  for (int learn = 1; learn >= 0; --learn)
    hipLaunchKernelGGL(bgs::asbl_lut_kernel, dim3(bgs::kAsblLutRows), dim3(bgs::kBlock), 0, e->stream(), st.lut + (learn ? 0 : one), learn, p.alpha_learn, 1 - p.alpha_learn,
                       p.alpha_detection, 1 - p.alpha_detection);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream()));
  st.lut_alpha[0] = p.alpha_learn, st.lut_alpha[1] = p.alpha_detection, st.lut_valid = true;
  return BGS_OK;
}

int asbl_allocate(bgs_engine* e) {
  AsblState& st = make_state<AsblState>(e);
  for (auto& b : st.bg) DMALLOC(b, e->n * e->S);
  st.flip.assign(e->S, 0);
  return asbl_build_lut(e);
}

uint64_t asbl_key(const bgs_engine* e, int i) {
  const bgs_params& p = e->p;
  return (uint64_t)(e->seen[i] == 0) | (uint64_t)asbl_of(e).flip[i] << 1 | (uint64_t)((p.learning_frames > 0 && e->counter[i] <= p.learning_frames) ? 4 : 0);
}

int asbl_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const int C = e->ch;
  const size_t npix = e->n * count, off = e->n * first;
  AsblState& st = asbl_of(e);
  const int cur = st.flip[first];
  for (int i = first; i < first + count; ++i)
    if (st.flip[i] != cur) return fail(BGS_ERR_INVALID, "streams %d and %d are not in lock-step", first, i);
  uint8_t* bufs[2] = {st.bg[0], st.bg[1]};
  if (e->seen[first] == 0) {  // img_input(gray).copyTo(img_background): a frame of threshold -1 ... simplest exact way is a tiny gray kernel
    bgs::FrameArgs a{};  // LAUNCH_FRAME_KERNEL reads `a`
    a.cur = d_frames, a.fg = bufs[cur] + off, a.npix = npix, a.enable_thr = 0;
    const int G = 1;
    LAUNCH_FRAME_KERNEL(gray_kernel, "gray_kernel");
  }
  bgs::AsblArgs q{};
  q.frame = d_frames, q.bg_in = bufs[cur] + off, q.bg_out = bufs[cur ^ 1] + off, q.fg = d_fg, q.bg_img = d_bg;
  q.rows = e->rows, q.cols = e->cols, q.thr = p.threshold;
  const int64_t cnt = e->counter[first];
  q.learn = (p.learning_frames > 0 && cnt <= p.learning_frames) ? 1 : 0;
  q.aL = p.alpha_learn, q.bL = 1 - p.alpha_learn, q.aD = p.alpha_detection, q.bD = 1 - p.alpha_detection;
  {
    Timed tm(e, s, "asbl_kernel");
    static const bool table = !(getenv("BGS_ASBL_TABLE") && atoi(getenv("BGS_ASBL_TABLE")) == 0);
    const uintptr_t ptrs = (uintptr_t)q.frame | (uintptr_t)q.bg_in | (uintptr_t)q.bg_out | (uintptr_t)q.fg | (uintptr_t)q.bg_img;
    // the table kernel moves whole dwords: rows of 4n pixels, aligned images (also the stream offset inside them: n % 4 == 0 then)
    if (table && e->cols % 4 == 0 && e->cols >= 4 && ptrs % 4 == 0) {
      // one wave per strip of 256 columns x R rows; 2 resident workgroups of 16 waves per CU (67 KB of LDS each): R such that the
      // strips of this launch fill them once, at least 8 rows (each strip re-reads the rows above and below it)
      const size_t waves = (size_t)2 * e->n_cu * (bgs::kAsbl2Block / bgs::kWave), nsx = (e->cols + bgs::kAsblSW - 1) / bgs::kAsblSW;
      const size_t blocks_y = std::max<size_t>(1, waves / ((size_t)count * nsx));
      const int R = (int)std::max<size_t>(8, (e->rows + blocks_y - 1) / blocks_y);
      const size_t nstrips = (size_t)count * nsx * ((e->rows + R - 1) / R), per_wg = bgs::kAsbl2Block / bgs::kWave;
      if (nstrips >= (1u << 31)) return fail(BGS_ERR_UNSUPPORTED, "AdaptiveSelectiveBackgroundLearning: launch too large");
      const dim3 grid((unsigned)std::min<size_t>((nstrips + per_wg - 1) / per_wg, (size_t)2 * e->n_cu));
      const uint8_t* lut = st.lut + (q.learn ? 0 : (size_t)bgs::kAsblLutRows * 256);
      if (C == 3)
        hipLaunchKernelGGL((bgs::asbl_stream_kernel<3>), grid, dim3(bgs::kAsbl2Block), 0, s, q, lut, count, R);
      else
        hipLaunchKernelGGL((bgs::asbl_stream_kernel<1>), grid, dim3(bgs::kAsbl2Block), 0, s, q, lut, count, R);
    } else {
      const dim3 grid((e->cols + bgs::kAsblTW - 1) / bgs::kAsblTW, (e->rows + bgs::kAsblTH - 1) / bgs::kAsblTH, count);
      if (C == 3)
        hipLaunchKernelGGL((bgs::asbl_kernel<3>), grid, dim3(bgs::kBlock), 0, s, q);
      else
        hipLaunchKernelGGL((bgs::asbl_kernel<1>), grid, dim3(bgs::kBlock), 0, s, q);
    }
  }
  if (d_bits) {
    if (!d_fg) return fail(BGS_ERR_UNSUPPORTED, "AdaptiveSelectiveBackgroundLearning: the packed mask is made from the byte mask, pass d_fg too");
    hipLaunchKernelGGL(bgs::mask_pack_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, (const uint8_t*)d_fg, d_bits, npix);
  }
  for (int i = first; i < first + count; ++i) {
    st.flip[i] = (uint8_t)(cur ^ 1);
    if (q.learn) e->counter[i]++;
  }
  *flags = BGS_FG_VALID | BGS_BG_VALID;
  return BGS_OK;
}

int64_t asbl_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  if (!strcmp(plane, "bg")) return copy_plane(plane, dst, cap, asbl_of(e).bg[asbl_of(e).flip[stream]] + e->n * stream, e->n);
  return unknown_plane(e, plane);
}

int asbl_apply_params(bgs_engine* e) {
  const AsblState& st = asbl_of(e);
  if (st.lut_valid && e->p.alpha_learn == st.lut_alpha[0] && e->p.alpha_detection == st.lut_alpha[1]) return BGS_OK;
  if (hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(BGS_ERR_HIP, "device sync failed");
  return asbl_build_lut(e);
}

constexpr Family kAsbl = [] {
  Family f{};
  f.allocate = asbl_allocate, f.key = asbl_key, f.run = asbl_run, f.get_state = asbl_get_state;
  f.apply_params = asbl_apply_params, f.needs_byte_mask = always, f.bg_channels = 1;
  return f;
}();
