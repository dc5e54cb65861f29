// engine_kde.h — the KDE engine (package_bgs/ae, BGS_KDE): model allocation, the host-built tables, the per-stream
// schedule of KDE::process and the state export.  Included by bgs_hip.hip inside its anonymous namespace; kernels in
// kernel_kde.h, layout and numeric contract in DESIGN.md §3 / §5.
//
// The per-stream counters mirror the reference object's members one for one:
//   fn    KDE::frameNumber           (learning frames while fn < framesToLearn, Estimation at fn == framesToLearn)
//   top   NPBGmodel::Top             (slot of the next learning frame)
//   tidx  NPBGSubtractor::TimeIndex  (update calls since the last Estimation; sampling events at tidx % rate == 0)
//   tbc   SequenceBGUpdate_Pairs' TBCount: a function-static in the reference, shared by every instance of a process
//         (DESIGN.md §5, quirk 2); here one per stream, restarted by bgs_reset_stream
//   tbtop NPBGmodel::TemporalBufferTop

struct KdeState : FamilyState {
  DevPtr<uint32_t> samples, tb, meta, acc;  // stream-major planes of 4-byte records (kernel_kde.h)
  DevPtr<double> lut;                       // the kernel table
  DevPtr<int2> gate;                        // the colour-ratio gate
  DevPtr<unsigned long long> trips;         // diagnostics: density-loop trips (BGS_KDE_TRIPS=1)
  uint64_t lanes = 0;                       // lanes the counted launches covered
  struct Stream {                           // the reference object's counters (above)
    int64_t fn = 0, top = 0, tidx = 0, tbc = 0, tbtop = 0;
  };
  std::vector<Stream> of;                   // one set per stream
};
KdeState& kde_of(const bgs_engine* e) { return state_of<KdeState>(e); }

int kde_tbl(const bgs_params& p) { return std::max(p.kde_time_window / p.kde_sequence_length, 2); }    // TemporalBufferLength
int kde_rate(const bgs_params& p) { return std::max(p.kde_time_window / p.kde_sequence_length, 2); }   // sampling period (same expression)

int kde_check(bgs_algo, const bgs_params& p) {
  if (p.kde_sequence_length < 3 || p.kde_sequence_length > 255)
    return fail(BGS_ERR_INVALID, "KDE SequenceLength must be 3..255 (PixelQTop and the histogram counts are bytes; below 3 medianCount is 0), got %d", p.kde_sequence_length);
  if (p.kde_frames_to_learn < 1) return fail(BGS_ERR_INVALID, "KDE framesToLearn must be >= 1, got %d", p.kde_frames_to_learn);
  if (p.kde_time_window < 1) return fail(BGS_ERR_INVALID, "KDE TimeWindowSize must be >= 1, got %d", p.kde_time_window);
  if (p.kde_time_window / p.kde_sequence_length > 255)
    return fail(BGS_ERR_INVALID, "KDE TimeWindowSize / SequenceLength must be <= 255 (TemporalBufferLength is a byte), got %d", p.kde_time_window / p.kde_sequence_length);
  return BGS_OK;
}

// KernelLUTable(255, 0.5, 36.5, 80) (KernelTable.cpp:60-116) in the reference's arithmetic, through the C library's exp.
void kde_kernel_table(std::vector<double>& tab) {
#pragma clang fp contract(off)
  const double PI = 3.14159, minsegma = 0.5, maxsegma = 36.5;
  const int half = bgs::kKdeHalf, bins = bgs::kKdeBins;
  tab.assign((size_t)bins * bgs::kKdeWidth, 0.0);
  const double segmastep = (maxsegma - minsegma) / bins;
  double segma = minsegma;
  for (int bin = 0; bin < bins; segma += segmastep, bin++) {
    const double C1 = 1 / (sqrt(2 * PI) * segma), C2 = -1 / (2 * segma * segma);
    double* row = tab.data() + (size_t)bin * bgs::kKdeWidth;
    double sum = 0;
    for (int x = 0; x <= half; x++) {
      const double y = x / 1.0, v = C1 * exp(C2 * y * y);
      row[half + x] = row[half - x] = v;
      sum += 2 * v;
    }
    sum -= C1;
    for (int x = 0; x <= half; x++) row[half + x] = row[half - x] = row[half + x] / sum;
  }
}

// The colour-ratio brightness gate (x1, x2) for every sample brightness g (NPBGSubtractor.cpp:966-985): a pure function of
// (g, alpha), so the kernel compares integers.
void kde_gate_table(double alpha, int2* out) {
#pragma clang fp contract(off)
  const double beta = 3.0, betau = 100.0, lo = 1 - alpha, hi = 1 + alpha;
  for (int g = 0; g < 256; ++g) {
    if (g < beta / alpha)
      out[g] = make_int2((int)(g - beta), (int)(g + beta));
    else if (g > betau / alpha)
      out[g] = make_int2((int)(g - betau), (int)(g + betau));
    else
      out[g] = make_int2((int)(g * lo + 0.5), (int)(g * hi + 0.5));
  }
}

int kde_allocate(bgs_engine* e) {
  const bgs_params& p = e->p;
  int rc = kde_check(e->algo, p);
  if (rc) return rc;
  if (e->ch == 1 && p.kde_color_ratios)
    return fail(BGS_ERR_UNSUPPORTED, "KDE colour ratios need 3-channel frames (BGR2SnGnRn reads 3 bytes per pixel of a gray frame: NPBGSubtractor.cpp:1141)");
  const size_t n = e->n, S = (size_t)e->S, SL = (size_t)p.kde_sequence_length, TBL = (size_t)kde_tbl(p);
  if (n * S >= (size_t)1 << 31) return fail(BGS_ERR_INVALID, "KDE: streams x pixels must stay below 2^31");
  KdeState& st = make_state<KdeState>(e);
  st.of.assign(S, KdeState::Stream());
  DMALLOC(st.samples, S * SL * n * 4);
  DMALLOC(st.tb, S * TBL * n * 4);
  DMALLOC(st.meta, S * n * 4);
  DMALLOC(st.acc, S * n * 4);
  DMALLOC(st.lut, (size_t)bgs::kKdeBins * bgs::kKdeWidth * sizeof(double));
  DMALLOC(st.gate, 256 * sizeof(int2));
  DMALLOC(st.trips, sizeof(unsigned long long));
  std::vector<double> tab;
  kde_kernel_table(tab);
  int2 gate[256];
  kde_gate_table(p.kde_alpha, gate);
  HIP_TRY(hipMemcpyAsync(st.lut, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, e->stream()));
  HIP_TRY(hipMemcpyAsync(st.gate, gate, sizeof(gate), hipMemcpyHostToDevice, e->stream()));
  HIP_TRY(hipMemsetAsync(st.trips, 0, sizeof(unsigned long long), e->stream()));
  HIP_TRY(hipStreamSynchronize(e->stream()));  // `tab` and `gate` leave scope
  return BGS_OK;
}

// What the next frame of stream i does: 0 learn, 1 Estimation + subtract, 2 subtract (KDE.cpp:74-88).
int kde_phase(const bgs_engine* e, int i) {
  const int64_t F = e->p.kde_frames_to_learn, fn = kde_of(e).of[i].fn;
  return fn < F ? 0 : fn == F ? 1 : 2;
}

// Everything the launch of stream i's next frame depends on (launch_key): first frame (model clear), phase, learning slot,
// temporal-buffer top and whether this update is a sampling event.
uint64_t kde_key(const bgs_engine* e, int i) {
  const KdeState::Stream& k = kde_of(e).of[i];
  const int ph = kde_phase(e, i);
  const int64_t tidx = ph == 1 ? 0 : k.tidx;  // Estimation restarts TimeIndex
  const bool sample = ph > 0 && tidx % kde_rate(e->p) == 0 && k.tbc >= kde_tbl(e->p);
  return (uint64_t)(e->seen[i] == 0) | (uint64_t)ph << 1 | (uint64_t)(ph == 0 ? k.top : 0) << 3 | (uint64_t)(ph ? k.tbtop : 0) << 11 | (uint64_t)sample << 19;
}

// One frame of KDE::process for streams [first, first+count), which share kde_key.
int kde_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t*, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const bgs_params& p = e->p;
  KdeState& st = kde_of(e);
  const size_t n = e->n, npix = n * count, SL = (size_t)p.kde_sequence_length, TBL = (size_t)kde_tbl(p);
  if (e->seen[first] == 0) {  // a new model (NPBGmodel's constructor: Sequence zero-filled); every plane cleared, run-contiguous
    HIP_TRY(hipMemsetAsync(st.samples + first * SL * n, 0, npix * SL * 4, s));
    HIP_TRY(hipMemsetAsync(st.tb + first * TBL * n, 0, npix * TBL * 4, s));
    HIP_TRY(hipMemsetAsync(st.meta + first * n, 0, npix * 4, s));
    HIP_TRY(hipMemsetAsync(st.acc + first * n, 0, npix * 4, s));
    for (int i = first; i < first + count; ++i) st.of[i] = KdeState::Stream();
  }
  bgs::KdeArgs a{};
  a.cur = d_frames, a.fg = d_fg, a.fg_bits = d_bits;
  a.samples = st.samples + first * SL * n, a.tb = st.tb + first * TBL * n, a.meta = st.meta + first * n, a.acc = st.acc + first * n;
  a.lut = st.lut, a.gate = st.gate, a.trips = e->knob.kde_count_trips ? st.trips.p : nullptr;
  a.npix = (uint32_t)npix, a.n = (uint32_t)n;
  a.th = p.kde_threshold, a.th_sum = p.kde_threshold * (double)SL;
  a.SL = (int)SL, a.TBL = (int)TBL, a.C = e->ch;
  a.mode = e->ch == 1 ? bgs::kKdeGray : p.kde_color_ratios ? bgs::kKdeRatios : bgs::kKdeRgb;
  a.sd_fixed = p.kde_sd_estimation ? -1 : (int)std::floor(((1.0 - 0.5) * bgs::kKdeBins) / (36.5 - 0.5));  // DEFAULTSEGMA's bin: 1
  a.xcd_swizzle = e->knob.xcd_swizzle >= 2;
  const KdeState::Stream k0 = st.of[first];
  const int ph = kde_phase(e, first);
  const dim3 grid(blocks_for(npix)), block(bgs::kBlock);
  *flags = 0;
  if (ph == 0) {  // AddFrame: no output (img_output untouched)
    a.top = (int)k0.top;
    hipLaunchKernelGGL(bgs::kde_learn_kernel, grid, block, 0, s, a);
    for (int i = first; i < first + count; ++i) st.of[i].fn++, st.of[i].top = (st.of[i].top + 1) % (int64_t)SL;
    return BGS_OK;
  }
  if (ph == 1) {  // Estimation
    hipLaunchKernelGGL(bgs::kde_estimate_kernel, grid, block, 0, s, a);
    for (int i = first; i < first + count; ++i) st.of[i].fn++, st.of[i].tidx = 0;
  }
  const KdeState::Stream& k = st.of[first];
  a.update = p.kde_update_model != 0;
  a.sample = k.tidx % kde_rate(p) == 0 && k.tbc >= (int64_t)TBL;
  a.tb_top = (int)k.tbtop, a.tb_next = (int)((k.tbtop + 1) % (int64_t)TBL);
  {
    Timed tm(e, s, "kde_frame_kernel");
    hipLaunchKernelGGL(bgs::kde_frame_kernel, grid, block, 0, s, a);
  }
  if (a.trips) st.lanes += npix;
  if (a.update)
    for (int i = first; i < first + count; ++i) {
      KdeState::Stream& q = st.of[i];
      q.tbtop = (q.tbtop + 1) % (int64_t)TBL, q.tbc++, q.tidx++;
    }
  *flags = BGS_FG_VALID;
  return BGS_OK;
}

// bgs_get_state planes: "samples" u8 [SL][n][C] in slot order, "sd_bins" u8 [n][C], "qtop" u8 [n], "acc" u32 [n];
// diagnostics "trips": u64 {density-loop trips, lanes} summed over every frame launch since creation (BGS_KDE_TRIPS=1).
int64_t kde_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const KdeState& st = kde_of(e);
  const size_t n = e->n, C = (size_t)e->ch, SL = (size_t)e->p.kde_sequence_length;
  const bool smp = !strcmp(plane, "samples"), sd = !strcmp(plane, "sd_bins"), qt = !strcmp(plane, "qtop");
  if (!strcmp(plane, "acc")) return copy_plane(plane, dst, cap, st.acc + (size_t)stream * n, n * 4);
  if (smp || sd || qt) {  // 4-byte records on the device, bytes for the caller
    const size_t words = smp ? SL * n : n, need = qt ? n : words * C;
    if (cap < need) return too_small(plane);
    std::vector<uint32_t> v(words);
    if (fetch(v.data(), (smp ? st.samples + (size_t)stream * SL * n : st.meta + (size_t)stream * n), words * 4)) return BGS_ERR_HIP;
    for (size_t r = 0; r < words; ++r) {
      if (qt) ((uint8_t*)dst)[r] = (uint8_t)(v[r] >> 24);
      else
        for (size_t c = 0; c < C; ++c) ((uint8_t*)dst)[r * C + c] = (uint8_t)(v[r] >> (8 * c));
    }
    return (int64_t)need;
  }
  if (!strcmp(plane, "trips")) {
    uint64_t rec[2] = {0, st.lanes};
    if (cap < sizeof(rec)) return too_small(plane);
    if (fetch(rec, st.trips, 8)) return BGS_ERR_HIP;
    return copy_host(plane, dst, cap, rec, sizeof(rec));
  }
  return unknown_plane(e, plane);
}

void kde_reset_stream(bgs_engine* e, int stream) { kde_of(e).of[stream] = KdeState::Stream(); }

// KDE.cpp:40-66: Intialize / SetThresholds once; framesToLearn is re-read every frame (and update_model is live)
void kde_keep_frozen(bgs_params& p, const bgs_params& old) {
  p.kde_sequence_length = old.kde_sequence_length, p.kde_time_window = old.kde_time_window, p.kde_sd_estimation = old.kde_sd_estimation;
  p.kde_color_ratios = old.kde_color_ratios, p.kde_threshold = old.kde_threshold, p.kde_alpha = old.kde_alpha;
}

constexpr Family kKde = [] {
  Family f{};
  f.check = kde_check, f.allocate = kde_allocate, f.key = kde_key, f.run = kde_run, f.get_state = kde_get_state;
  f.reset_stream = kde_reset_stream, f.keep_frozen = kde_keep_frozen;
  return f;
}();
