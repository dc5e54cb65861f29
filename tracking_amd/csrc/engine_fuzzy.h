// engine_fuzzy.h — host side of package_bgs/tb FuzzySugenoIntegral / FuzzyChoquetIntegral (BGS_FUZZY_SUGENO / BGS_FUZZY_CHOQUET): the
// refusals, the LBP table, allocation, the per-stream learn / detect schedule and the state export.  Included by bgs_hip.hip inside
// its anonymous namespace; kernels in kernel_fuzzy.h.
//
// The wrapper re-reads its XML on every frame and every one of the seven values acts on that frame (Fuzzy*Integral.cpp:39, :191-205),
// so bgs_set_fuzzy_params replaces them all, between any two frames.  frameNumber is the object's own counter: kept per stream, and
// `frameNumber <= framesToLearn` is evaluated per stream and per frame, so streams of different ages share every launch (per-stream
// bits) and raising frames_to_learn mid-run sends a detecting stream back to learning, as it would the wrapper.

struct FuzzyState : FamilyState {
  DevPtr<float> bg;      // the float BGR background [S][n][3]
  DevPtr<float> f;       // per-frame scratch: seven planes [S][n] (gray of input and background, hs[3], integral column-major, blurred integral row-major)
  DevPtr<float> tab;     // the LBP table
  DevPtr<uint8_t> code, bprod;       // pi codes, scan block products
  DevPtr<uint32_t> minmax;           // per-stream min / max keys
  std::vector<int64_t> fn;           // frameNumber of each stream's object
  std::vector<uint8_t> detected;     // the stream has an integral image
};
FuzzyState& fz_of(const bgs_engine* e) { return state_of<FuzzyState>(e); }

const char* fz_name(bgs_algo a) { return a == BGS_FUZZY_SUGENO ? "FuzzySugenoIntegral" : "FuzzyChoquetIntegral"; }

void fz_defaults(bgs_fuzzy_params* p) {  // Fuzzy*Integral.cpp:20-21
  std::memset(p, 0, sizeof(*p));
  p->struct_size = (uint32_t)sizeof(*p);
  p->frames_to_learn = 10, p->alpha_learn = 0.1, p->alpha_update = 0.01, p->color_space = 1, p->option = 2, p->smooth = 1, p->threshold = 0.67;
}

// Needs no device: checked before the GPU is opened.
int fz_check(bgs_algo algo, const bgs_fuzzy_params& p) {
  const char* nm = fz_name(algo);
  if (p.color_space == 2)
    return fail(BGS_ERR_UNSUPPORTED, "%s: colorSpace 2 (Ohta) is not built: I2 = (R-B)/2 is 0 wherever R == B, the ratio with a negative value is -inf, and the whole background is NaN after the first detecting frame", nm);
  if (p.color_space == 3 || p.color_space == 4) return fail(BGS_ERR_UNSUPPORTED, "%s: colorSpace %d needs OpenCV's float cvCvtColor, which is not built", nm, p.color_space);
  if (p.color_space != 1) return fail(BGS_ERR_UNSUPPORTED, "%s: colorSpace %d is none of 1..4", nm, p.color_space);
  if (p.option != 1 && p.option != 2) return fail(BGS_ERR_UNSUPPORTED, "%s: option %d runs neither branch: the reference's integral image is uninitialised memory", nm, p.option);
  if (p.frames_to_learn < 0) return fail(BGS_ERR_INVALID, "%s: framesToLearn %d < 0 (the first frame would detect against an empty background)", nm, p.frames_to_learn);
  return BGS_OK;
}
int fz_check_geometry(bgs_algo algo, int rows, int cols, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "%s reads 3-channel frames only (cvtColor(CV_BGR2GRAY) asserts on 1 channel, %s.cpp:79)", fz_name(algo), fz_name(algo));
  if (rows < 2 || cols < 2) return fail(BGS_ERR_UNSUPPORTED, "%s: a %dx%d frame is narrower or lower than 2 pixels (the LBP of pixel (0,0) reads outside it)", fz_name(algo), cols, rows);
  return BGS_OK;
}

// The interior LBP: v = fl32(v + (bit_l * 2^l) / 255.0) over the nine slots, the term a double (FuzzyUtils.cpp:148-150): 256 values.
// Then the corner's eight: fl32((2 b1 + 4 b2 + 8 b3) / 255.0) (:54).
void fz_table(float* tab) {
  const float carre[9] = {1, 2, 4, 8, 0, 16, 32, 64, 128};
  for (int code = 0; code < 256; ++code) {
    float v = 0;
    for (int l = 0; l < 9; ++l) {
      const float bit = l == 4 ? 1.0f : (float)((code >> (l < 4 ? l : l - 1)) & 1);
      v = (float)((double)v + (double)(bit * carre[l]) / 255.0);
    }
    tab[code] = v;
  }
  for (int k = 0; k < 8; ++k) tab[256 + k] = (float)((double)(2 * k) / 255.0);
}

uint64_t fz_key(const bgs_engine*, int) { return 0; }  // learn / first-frame go into the launches as per-stream bits

int fz_allocate(bgs_engine* e) {
  int rc = fz_check(e->algo, e->fz);
  if (rc) return rc;
  const size_t n = e->n, S = (size_t)e->S, nb = (n + bgs::kFzScan - 1) / bgs::kFzScan;
  if (n * S * 3 >= (size_t)1 << 31) return fail(BGS_ERR_INVALID, "%s: streams x pixels x 3 must stay below 2^31", fz_name(e->algo));
  FuzzyState& st = make_state<FuzzyState>(e);
  DMALLOC(st.bg, S * n * 3 * sizeof(float));
  DMALLOC(st.f, S * n * 7 * sizeof(float));  // gray_in, gray_bg, hs[3], iq, I
  DMALLOC(st.code, S * n);
  DMALLOC(st.bprod, S * nb);
  DMALLOC(st.minmax, S * 2 * sizeof(uint32_t));
  DMALLOC(st.tab, 264 * sizeof(float));
  float tab[264];
  fz_table(tab);
  HIP_TRY(hipMemcpyAsync(st.tab, tab, sizeof(tab), hipMemcpyHostToDevice, e->stream()));
  HIP_TRY(hipStreamSynchronize(e->stream()));  // `tab` leaves scope
  st.fn.assign(S, 0);
  st.detected.assign(S, 0);
  return BGS_OK;
}

// One frame of Fuzzy*Integral::process for streams [first, first+count).
int fz_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  FuzzyState& fs = fz_of(e);
  const size_t n = e->n, P = n * (size_t)e->S;
  const bgs_fuzzy_params& p = e->fz;
  const uint32_t nb = (uint32_t)((n + bgs::kFzScan - 1) / bgs::kFzScan);
  if (d_bits && !d_fg) return fail(BGS_ERR_INVALID, "internal: the fuzzy integrals' packed mask needs a byte mask");  // process_range provides one
  uint32_t all = BGS_FG_VALID | BGS_BG_VALID;
  for (int f = 0; f < count; f += bgs::kFzStreams) {
    const int c = std::min(bgs::kFzStreams, count - f);
    const size_t o = (size_t)f * n, so = (size_t)(first + f) * n;
    bgs::FzArgs a{};
    a.cur = d_frames + o * 3, a.fg = d_fg ? d_fg + o : nullptr, a.bgout = d_bg ? d_bg + o * 3 : nullptr;
    a.bg = fs.bg + so * 3;
    a.gray_in = fs.f + so, a.gray_bg = fs.f + P + so, a.hs = fs.f + 2 * P + so, a.iq = fs.f + 5 * P + so, a.I = fs.f + 6 * P + so;
    a.plane = P, a.code = fs.code + so, a.bprod = fs.bprod + (size_t)(first + f) * nb, a.minmax = fs.minmax + (size_t)(first + f) * 2;
    a.tab = fs.tab, a.n = (uint32_t)n, a.nb = nb, a.W = e->cols, a.H = e->rows;
    a.a_learn = (float)p.alpha_learn, a.b_learn = (float)(1 - p.alpha_learn);
    a.a_update = (float)p.alpha_update, a.thr = (float)p.threshold;
    if (p.option == 1) a.G[0] = 0.4f, a.G[1] = 0.3f, a.G[2] = 0.3f;  // FuzzyMeasureG, Fuzzy*Integral.cpp:109 / :116
    else a.G[0] = 0.6f, a.G[1] = 0.3f, a.G[2] = 0.1f;
    a.choquet = e->algo == BGS_FUZZY_CHOQUET, a.colours = a.choquet && p.option == 1, a.smooth = p.smooth != 0;
    int detecting = 0;
    for (int i = 0; i < c; ++i) {
      const int st = first + f + i;
      if (e->seen[st] == 0) fs.fn[st] = 0, fs.detected[st] = 0, a.init_mask |= (uint64_t)1 << i;  // a new object: img_background_f3 is empty
      const bool learn = fs.fn[st] <= (int64_t)p.frames_to_learn;            // if(frameNumber <= framesToLearn)
      if (learn) a.learn_mask |= (uint64_t)1 << i;
      else ++detecting, fs.detected[st] = 1;
      e->last_flags[st] = learn ? 0u : (uint32_t)(BGS_FG_VALID | BGS_BG_VALID);  // per_stream_flags: learning and detecting streams share the run
      all &= e->last_flags[st];
      fs.fn[st]++;
    }
    const uint32_t npix = (uint32_t)(n * c);
    Timed tm(e, s, detecting ? "fuzzy_frame (prep, pixel, scan block / top / apply, median, update)" : "fuzzy_prep_kernel (learning)");
    hipLaunchKernelGGL(bgs::fuzzy_prep_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, a, npix);
    if (!detecting) continue;
    const dim3 tiles((e->cols + bgs::kFzTile - 1) / bgs::kFzTile, (e->rows + bgs::kFzTile - 1) / bgs::kFzTile, c), tile(bgs::kFzTile, bgs::kFzTile);
    hipLaunchKernelGGL(bgs::fuzzy_pixel_kernel, tiles, tile, 0, s, a);
    hipLaunchKernelGGL(bgs::fuzzy_scan_block_kernel, dim3(nb, c), dim3(bgs::kBlock), 0, s, a);
    hipLaunchKernelGGL(bgs::fuzzy_scan_top_kernel, dim3(c), dim3(bgs::kFzTop), 0, s, a);
    hipLaunchKernelGGL(bgs::fuzzy_apply_kernel, dim3(nb, c), dim3(bgs::kBlock), 0, s, a);
    hipLaunchKernelGGL(bgs::fuzzy_median_kernel, tiles, tile, 0, s, a);
    hipLaunchKernelGGL(bgs::fuzzy_update_kernel, dim3(blocks_for(npix)), dim3(bgs::kBlock), 0, s, a, npix);
  }
  if (d_bits && (any_flags(e, first, count) & BGS_FG_VALID))  // n % 64 == 0 here; the words of a learning stream are as undefined as its byte mask
    hipLaunchKernelGGL(bgs::mask_pack_kernel, dim3(blocks_for(n * count)), dim3(bgs::kBlock), 0, s, (const uint8_t*)d_fg, d_bits, n * count);
  *flags = all;
  return BGS_OK;
}

// bgs_get_state planes (include/bgs_hip.h)
int64_t fz_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const FuzzyState& st = fz_of(e);
  const size_t n = e->n, P = n * (size_t)e->S;
  if (!strcmp(plane, "count")) {
    const int64_t v = e->seen[stream] == 0 ? 0 : st.fn[stream];
    return copy_host(plane, dst, cap, &v, 8);
  }
  const bool bgp = !strcmp(plane, "background"), ip = !strcmp(plane, "integral"), mp = !strcmp(plane, "minmax");
  if (!bgp && !ip && !mp) return unknown_plane(e, plane);
  if (e->seen[stream] == 0) return fail(BGS_ERR_STATE, "stream %d has no background yet", stream);
  if ((ip || mp) && !st.detected[stream]) return fail(BGS_ERR_STATE, "stream %d has not detected yet: no integral image", stream);
  if (bgp) return copy_plane(plane, dst, cap, st.bg + (size_t)stream * n * 3, n * 12);
  if (ip) return copy_plane(plane, dst, cap, st.f + 6 * P + (size_t)stream * n, n * 4);
  uint32_t k[2];
  if (cap < 8) return too_small(plane);
  if (fetch(k, st.minmax + (size_t)stream * 2, 8)) return BGS_ERR_HIP;
  for (uint32_t& b : k) b ^= (b >> 31) ? 0x80000000u : 0xffffffffu;
  return copy_host(plane, dst, cap, k, 8);
}

void fz_reset_stream(bgs_engine* e, int stream) { fz_of(e).fn[stream] = 0, fz_of(e).detected[stream] = 0; }

constexpr Family kFuzzy = [] {
  Family f{};
  f.check_geometry = fz_check_geometry, f.allocate = fz_allocate, f.key = fz_key, f.run = fz_run, f.get_state = fz_get_state;
  f.reset_stream = fz_reset_stream, f.needs_byte_mask = always, f.per_stream_flags = true;
  return f;
}();
// live: all seven act on the next frame, the host fills its launch arguments from them
constexpr ParamBlock<bgs_fuzzy_params> kFuzzyBlock{&bgs_engine::fz, &kFuzzy, "bgs_fuzzy_params", "FuzzySugenoIntegral / FuzzyChoquetIntegral", fz_defaults, fz_check, true};
