// engine_gmg.h — host side of GMG (BGS_GMG; kernel_gmg.h).  Included by bgs_hip.hip inside its anonymous namespace.

struct GmgState : FamilyState {
  DevPtr<int2> rec;                  // {colour, weight} histogram records [F][P] (kernel_gmg.h)
  DevPtr<uint8_t> nfeat, raw_mask;   // features per pixel [P]; the mask before the median filter [P]
};
GmgState& gmg_of(const bgs_engine* e) { return state_of<GmgState>(e); }

int gmg_check(bgs_algo, const bgs_params& p) {
  if (p.gmg_max_features < 1 || p.gmg_max_features > 64) return fail(BGS_ERR_UNSUPPORTED, "GMG maxFeatures must be 1..64, got %d", p.gmg_max_features);
  if (p.gmg_smoothing_radius != 0 && (p.gmg_smoothing_radius < 3 || p.gmg_smoothing_radius > 15 || p.gmg_smoothing_radius % 2 == 0))
    return fail(BGS_ERR_UNSUPPORTED, "GMG smoothingRadius (cv::medianBlur kernel) must be 0 or odd 3..15, got %d", p.gmg_smoothing_radius);
  return BGS_OK;
}

int gmg_allocate(bgs_engine* e) {
  const size_t P = e->n * e->S, F = (size_t)e->p.gmg_max_features;
  GmgState& st = make_state<GmgState>(e);
  DMALLOC(st.raw_mask, P);
  DMALLOC(st.rec, P * F * sizeof(int2));
  DMALLOC(st.nfeat, P);
  return BGS_OK;
}

uint64_t gmg_key(const bgs_engine* e, int i) {
  const int64_t t = e->seen[i];
  return (uint64_t)(t == 0) | (uint64_t)(t >= e->p.gmg_init_frames) << 1 | (uint64_t)(t == (int64_t)e->p.gmg_init_frames - 1) << 2;
}

int gmg_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t*, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  const GmgState& st = gmg_of(e);
  const int64_t t = e->seen[first];
  const size_t npix = e->n * count, off = e->n * first;
  if (d_bits && !d_fg) return fail(BGS_ERR_UNSUPPORTED, "GMG: the packed mask is made from the byte mask, pass d_fg too");
  const size_t P = e->n * e->S;
  if (t == 0) hipLaunchKernelGGL(bgs::gmg_clear_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, st.nfeat + off, npix);  // initialize(): nfeatures = 0
  bgs::GmgArgs g{};
  g.frame = d_frames, g.raw = st.raw_mask + off, g.rec = st.rec, g.nfeat = st.nfeat;
  g.plane = P, g.state_off = off, g.npix = npix, g.F = p.gmg_max_features, g.C = e->ch, g.levels = p.gmg_quantization_levels;
  g.typical = t >= p.gmg_init_frames, g.update = p.gmg_update_background_model != 0, g.normalize_now = t == (int64_t)p.gmg_init_frames - 1;
  // a decayed weight goes back as the whole 8-byte record (512 contiguous bytes per wave) rather than as a 4-byte store into it
  // (every other dword of the line: partial sectors): 0.294 -> 0.281 ms per 8 x 1080p, same box, alternating; BGS_GMG_FULL_STORE=0: the 4-byte stores
  static const bool gmg_full = !(getenv("BGS_GMG_FULL_STORE") && atoi(getenv("BGS_GMG_FULL_STORE")) == 0);
  g.fullStore = gmg_full ? 1 : 0;
  g.lr = p.gmg_learning_rate, g.prior = p.gmg_background_prior, g.thr = p.gmg_decision_threshold;
  {
    Timed tm(e, s, "gmg_kernel");
    hipLaunchKernelGGL(bgs::gmg_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, g);
  }
  if (d_fg) {
    if (p.gmg_smoothing_radius > 0) {  // cv::medianBlur(fgmask, smoothingRadius) of a {0,255} mask
      bgs::MorphArgs m{st.raw_mask + off, d_fg, e->rows, e->cols, 3, p.gmg_smoothing_radius};
      bgs::morph_launch(m, (int)count, s);
    } else {
      HIP_TRY(hipMemcpyAsync(d_fg, st.raw_mask + off, npix, hipMemcpyDeviceToDevice, s));
    }
    if (d_bits) hipLaunchKernelGGL(bgs::mask_pack_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, (const uint8_t*)d_fg, d_bits, npix);
  }
  *flags = BGS_FG_VALID;  // no getBackgroundImage for GMG (GMG.cpp:59): img_bgmodel ends up empty
  return BGS_OK;
}

// canonical: colors int32 [F][n], weights f32 [F][n] (entries past the count exported as 0), nfeatures int32 [n]; "bg": the unsmoothed mask
int64_t gmg_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const GmgState& st = gmg_of(e);
  const size_t n = e->n, P = n * e->S, off = n * stream, F = (size_t)e->p.gmg_max_features;
  const bool nfp = !strcmp(plane, "nfeatures"), cw = !strcmp(plane, "colors") || !strcmp(plane, "weights");
  if (!strcmp(plane, "bg")) return copy_plane(plane, dst, cap, st.raw_mask + off, n);
  if (!nfp && !cw) return unknown_plane(e, plane);
  if (cap < (nfp ? n * 4 : n * F * 4)) return too_small(plane);
  std::vector<uint8_t> nf(n);
  if (fetch(nf.data(), st.nfeat + off, n)) return BGS_ERR_HIP;
  if (nfp) {
    for (size_t i = 0; i < n; ++i) ((int32_t*)dst)[i] = nf[i];
    return (int64_t)(n * 4);
  }
  const int which = !strcmp(plane, "colors") ? 0 : 1;  // the device holds {colour, weight} records (kernel_gmg.h)
  std::vector<uint32_t> recs(n * 2);
  for (size_t f = 0; f < F; ++f) {
    if (fetch(recs.data(), st.rec + f * P + off, n * 8)) return BGS_ERR_HIP;
    for (size_t i = 0; i < n; ++i) ((uint32_t*)dst)[f * n + i] = f >= nf[i] ? 0u : recs[2 * i + which];
  }
  return (int64_t)(n * F * 4);
}

void gmg_keep_frozen(bgs_params& p, const bgs_params& old) { p.gmg_max_features = old.gmg_max_features; }  // sizes the histogram planes

constexpr Family kGmg = [] {
  Family f{};
  f.check = gmg_check, f.allocate = gmg_allocate, f.key = gmg_key, f.run = gmg_run, f.get_state = gmg_get_state;
  f.keep_frozen = gmg_keep_frozen, f.needs_byte_mask = always;
  return f;
}();
