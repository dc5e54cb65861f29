// engine_dp2.h — host side of DPPratiMediodBGS (BGS_DP_PRATI_MEDIOD) and DPTextureBGS (BGS_DP_TEXTURE): checks, model allocation,
// the per-stream schedule and the state export.  Included by bgs_hip.hip inside its anonymous namespace; kernels in kernel_dp2.h.
//
// PratiMediod's buffer position and sample count are the same for every pixel of a stream (the wrapper clears the update mask
// every frame, PratiMediodBGS.cpp:80), and both follow from the stream's frame number t (bgs_engine::seen, restarted by
// bgs_reset_stream): frames 0, r, 2r, ... are sampled, so k = ceil(t / |r|) samples were offered before frame t, the buffer holds
// min(k, H) and a full one replaces slot (k - H) mod H next.  C's `t % r == 0` is the same test for a negative rate.

int dp2_check(bgs_algo algo, const bgs_params& p) {
  if (algo != BGS_DP_PRATI_MEDIOD) return BGS_OK;
  if (p.dp_sampling_rate == 0) return fail(BGS_ERR_UNSUPPORTED, "PratiMediod samplingRate 0 (frame_num %% 0)");
  if (p.dp_history_size < 1 || p.dp_history_size > BGS_PRATI_MAX_HISTORY)
    return fail(BGS_ERR_UNSUPPORTED, "PratiMediod historySize must be 1..%d (the kernel's 16-bit distance sums), got %d", BGS_PRATI_MAX_HISTORY, p.dp_history_size);
  if (!(p.dp_threshold >= 0)) return fail(BGS_ERR_UNSUPPORTED, "PratiMediod threshold must be >= 0 (the reference's unsigned LowThreshold wraps a negative one), got %g", (double)p.dp_threshold);
  return BGS_OK;
}

struct PratiState : FamilyState {
  DevPtr<uint32_t> samples, med;  // samples [S][H][n], medoid ping-pong [2][S][n]
  DevPtr<uint16_t> dist;          // [S][H][n]
};
struct TexState : FamilyState {
  DevPtr<uint32_t> r, gb;  // histogram planes [S][16][n], [S][32][n]
  DevPtr<uint8_t> mask;    // the last frame's mask [S][n] (the transposed update gate)
};
PratiState& prati_of(const bgs_engine* e) { return state_of<PratiState>(e); }
TexState& tex_of(const bgs_engine* e) { return state_of<TexState>(e); }

struct PratiSched {
  int cnt, pos, par;  // samples in the buffer, the slot a full buffer replaces, which median plane is current
  bool sample, masks;
};

PratiSched prati_sched(const bgs_engine* e, int i) {
  const int64_t t = e->seen[i], r = std::llabs((long long)e->p.dp_sampling_rate), H = e->p.dp_history_size;
  const int64_t k = t == 0 ? 0 : (t - 1) / r + 1;  // sampled frames before frame t
  PratiSched q;
  q.cnt = (int)std::min(k, H), q.pos = k >= H ? (int)((k - H) % H) : 0, q.par = (int)(k & 1);
  q.sample = t % e->p.dp_sampling_rate == 0, q.masks = t >= H;
  return q;
}

uint64_t dp2_key(const bgs_engine* e, int i) {
  if (e->algo == BGS_DP_TEXTURE) return e->seen[i] == 0;
  const PratiSched q = prati_sched(e, i);
  return (uint64_t)q.cnt | (uint64_t)q.pos << 8 | (uint64_t)q.par << 16 | (uint64_t)q.sample << 17 | (uint64_t)q.masks << 18;
}

int dp2_allocate(bgs_engine* e) {
  if (e->ch != 3) return fail(BGS_ERR_UNSUPPORTED, "the dp/ models read RgbImage pixels: 3-channel frames only (dp/Image.h:257-265)");
  const size_t n = e->n, S = (size_t)e->S;
  if (n * S >= (size_t)1 << 31) return fail(BGS_ERR_INVALID, "dp: streams x pixels must stay below 2^31");
  if (e->algo == BGS_DP_PRATI_MEDIOD) {
    const size_t H = (size_t)e->p.dp_history_size;
    PratiState& st = make_state<PratiState>(e);
    DMALLOC(st.samples, S * H * n * 4);
    DMALLOC(st.dist, S * H * n * 2);
    DMALLOC(st.med, 2 * S * n * 4);
  } else {
    TexState& st = make_state<TexState>(e);
    DMALLOC(st.r, S * 16 * n * 4);
    DMALLOC(st.gb, S * 32 * n * 4);
    DMALLOC(st.mask, S * n);
  }
  // Nothing is initialised here: a stream's first frame clears its planes on the launch stream (dp2_run)
  return BGS_OK;
}

// One frame of DPPratiMediodBGS::process / DPTextureBGS::process for streams [first, first+count), which share dp2_key.
int dp2_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t*, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const size_t n = e->n, npix = n * count, S = (size_t)e->S;
  const bool fresh = e->seen[first] == 0;
  if (e->algo == BGS_DP_PRATI_MEDIOD) {
    const bgs_params& p = e->p;
    const PratiState& st = prati_of(e);
    const size_t H = (size_t)p.dp_history_size;
    if (fresh) {  // new MEDIAN_BUFFERs: empty (the planes read as 0 until filled: bgs_get_state)
      HIP_TRY(hipMemsetAsync(st.samples + first * H * n, 0, npix * H * 4, s));
      HIP_TRY(hipMemsetAsync(st.dist + first * H * n, 0, npix * H * 2, s));
      for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(st.med + k * S * n + first * n, 0, npix * 4, s));
    }
    const PratiSched q = prati_sched(e, first);
    bgs::PratiArgs a{};
    a.cur = d_frames, a.fg = d_fg, a.fg_bits = d_bits;
    a.samples = st.samples + first * H * n, a.dist = st.dist + first * H * n;
    a.med_in = st.med + q.par * S * n + first * n, a.med_out = st.med + (q.par ^ 1) * S * n + first * n;
    a.npix = (uint32_t)npix, a.n = (uint32_t)n, a.rows = e->rows, a.cols = e->cols, a.H = (int)H;
    a.cnt = q.cnt, a.pos = q.pos, a.sample = q.sample, a.masks = q.masks;
    // dist (a byte) > LowThreshold as unsigned ints, HighThreshold = 2 * LowThreshold (DPPratiMediodBGS.cpp:57-58)
    const double lo = std::floor((double)p.dp_threshold);
    a.low = (int)std::min(lo, 255.0), a.high = (int)std::min(2 * lo, 255.0);
    Timed tm(e, s, "prati_kernel");
    hipLaunchKernelGGL(bgs::prati_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, a);
  } else {
    const TexState& st = tex_of(e);
    uint32_t* hr = st.r + first * 16 * n;
    uint32_t* hgb = st.gb + first * 32 * n;
    uint8_t* mask = st.mask + first * n;
    if (fresh) {  // pixels outside the interior keep 0 (the reference leaves them uninitialised and never reads them)
      HIP_TRY(hipMemsetAsync(hr, 0, npix * 16 * 4, s));
      HIP_TRY(hipMemsetAsync(hgb, 0, npix * 32 * 4, s));
    }
    bgs::TexArgs a{};
    a.cur = d_frames, a.fg = d_fg, a.mask = mask, a.hist_r = hr, a.hist_gb = hgb;
    a.n = (uint32_t)n, a.rows = e->rows, a.cols = e->cols, a.ws = (e->cols + 3) & ~3;
    a.tiles_x = (e->cols + bgs::kTexTW - 1) / bgs::kTexTW;
    a.tiles_per_img = a.tiles_x * ((e->rows + bgs::kTexTH - 1) / bgs::kTexTH);
    a.init = fresh;
    const dim3 grid((unsigned)((size_t)a.tiles_per_img * count)), block(bgs::kBlock);
    {
      Timed tm(e, s, "tex_compare_kernel");
      hipLaunchKernelGGL(bgs::tex_compare_kernel, grid, block, 0, s, a);
    }
    // on the first frame the model is this frame's histogram: the update is the identity there (bg + floor(0 + 1/2))
    if (!fresh) hipLaunchKernelGGL(bgs::tex_update_kernel, grid, block, 0, s, a);
    if (d_bits) hipLaunchKernelGGL(bgs::mask_pack_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, (const uint8_t*)mask, d_bits, npix);
  }
  *flags = BGS_FG_VALID;  // img_bgmodel is never written by the dp wrappers
  return BGS_OK;
}

// bgs_get_state planes (include/bgs_hip.h): PratiMediod "samples" u8 [H][n][3], "dist" u16 [H][n], "median" u8 [n][3], "count"
// int64 [2]; Texture "hist" u8 [n][3][64] (r, g, b).
int64_t dp2_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const size_t n = e->n, S = (size_t)e->S;
  if (e->algo == BGS_DP_PRATI_MEDIOD) {
    const PratiState& st = prati_of(e);
    const size_t H = (size_t)e->p.dp_history_size;
    const PratiSched q = prati_sched(e, stream);
    if (!strcmp(plane, "count")) {
      const int64_t v[2] = {q.cnt, q.pos};
      return copy_host(plane, dst, cap, v, 16);
    }
    if (!strcmp(plane, "dist")) return copy_plane(plane, dst, cap, st.dist + (size_t)stream * H * n, H * n * 2);
    const bool smp = !strcmp(plane, "samples"), med = !strcmp(plane, "median");
    if (smp || med) {
      const size_t words = smp ? H * n : n;
      if (cap < words * 3) return too_small(plane);
      std::vector<uint32_t> v(words);
      const uint32_t* src = smp ? st.samples + (size_t)stream * H * n : st.med + (size_t)q.par * S * n + (size_t)stream * n;
      if (fetch(v.data(), src, words * 4)) return BGS_ERR_HIP;
      for (size_t r = 0; r < words; ++r)
        for (int c = 0; c < 3; ++c) ((uint8_t*)dst)[r * 3 + c] = (uint8_t)(v[r] >> (8 * c));
      return (int64_t)(words * 3);
    }
  } else if (!strcmp(plane, "hist")) {
    const TexState& st = tex_of(e);
    if (cap < n * 192) return too_small(plane);
    std::vector<uint32_t> r(16 * n), gb(32 * n);
    if (fetch(r.data(), st.r + (size_t)stream * 16 * n, r.size() * 4) || fetch(gb.data(), st.gb + (size_t)stream * 32 * n, gb.size() * 4)) return BGS_ERR_HIP;
    uint8_t* o = (uint8_t*)dst;
    for (size_t i = 0; i < n; ++i)
      for (int b = 0; b < 192; ++b) {
        const int h = b >> 6, bin = b & 63;
        const uint32_t w = h == 0 ? r[(size_t)(bin >> 2) * n + i] : gb[(size_t)((h - 1) * 16 + (bin >> 2)) * n + i];
        o[i * 192 + b] = (uint8_t)(w >> (8 * (bin & 3)));
      }
    return (int64_t)(n * 192);
  }
  return unknown_plane(e, plane);
}

// PratiMediodBGS::Initalize copies m_params once (DPPratiMediodBGS.cpp:55-64)
void prati_keep_frozen(bgs_params& p, const bgs_params& old) {
  p.dp_threshold = old.dp_threshold, p.dp_sampling_rate = old.dp_sampling_rate;
  p.dp_history_size = old.dp_history_size, p.dp_weight = old.dp_weight;
}

constexpr Family kDpTexture = [] {
  Family f{};
  f.check = dp2_check, f.allocate = dp2_allocate, f.key = dp2_key, f.run = dp2_run, f.get_state = dp2_get_state;
  return f;
}();

constexpr Family kDpPratiMediod = [] {
  Family f = kDpTexture;
  f.keep_frozen = prati_keep_frozen;
  return f;
}();
