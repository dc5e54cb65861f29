// engine_eigen.h — host side of package_bgs/dp DPEigenbackgroundBGS (BGS_DP_EIGENBACKGROUND; kernel_eigen.h); included inside
// bgs_hip.hip's anonymous namespace.
//
// The wrapper re-reads its XML on every frame, but the three values reach the params object once, `if(firstTime)`
// (DPEigenbackgroundBGS.cpp:45-66): they are taken when the geometry is set and a later bgs_set_eigen_params leaves them in force.
// LowThreshold() is a float&, HighThreshold() = 2 * LowThreshold().  frame_num is the wrapper's own counter = the stream's `seen`:
// frames 0 .. H-1 fill the history, frame H builds the model in front of its own detection, Update() is empty, so the model never
// changes after that.  Everything is enqueued on the caller's stream; nothing here waits for the device.

struct EigenState : FamilyState {
  DevPtr<uint8_t> hist;             // [S][H][Lp]
  DevPtr<float> avg, E, coeff;      // [S][Lp], [S][M][Lp], [S][M]
  DevPtr<unsigned long long> G;     // [S][H][H]
  DevPtr<double> W, lam, slab;      // [S][M][H], [S][H], [S][chunks][M]
  int H = 0, M = 0;
  uint32_t L = 0, Lp = 0, chunks = 0;
  float low = 0, high = 0;
};
EigenState& eig_of(const bgs_engine* e) { return state_of<EigenState>(e); }

constexpr const char* kEigName = "DPEigenbackground";

void eig_defaults(bgs_eigen_params* p) {  // DPEigenbackgroundBGS.cpp:19
  std::memset(p, 0, sizeof(*p));
  p->struct_size = (uint32_t)sizeof(*p);
  p->threshold = 225, p->history_size = 20, p->embedded_dim = 10;
}

// Needs no device: checked before the GPU is opened.
int eig_check(bgs_algo, const bgs_eigen_params& p) {
  if (p.history_size < 2 || p.history_size > BGS_EIGEN_MAX_HISTORY)
    return fail(BGS_ERR_UNSUPPORTED, "%s: historySize %d is outside 2..%d", kEigName, p.history_size, BGS_EIGEN_MAX_HISTORY);
  // centred data has rank <= H - 1: at embeddedDim == historySize the reference projects onto a normalised rounding residue, above it OpenCV asserts
  if (p.embedded_dim < 1 || p.embedded_dim > p.history_size - 1)
    return fail(BGS_ERR_UNSUPPORTED, "%s: embeddedDim %d is outside 1..historySize - 1 = %d (centred data has rank <= historySize - 1)", kEigName, p.embedded_dim, p.history_size - 1);
  return BGS_OK;
}
int eig_check_geometry(bgs_algo, int, int, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "%s reads RgbImage pixels: 3-channel frames only (dp/Image.h:257-265)", kEigName);
  return BGS_OK;
}

int eig_allocate(bgs_engine* e) {
  const bgs_eigen_params& p = e->eig;  // the defaults or what passed eig_check in bgs_set_eigen_params
  const size_t S = (size_t)e->S, L = e->n * 3;
  if (L >= (size_t)1 << 31) return fail(BGS_ERR_INVALID, "%s: pixels x 3 must stay below 2^31", kEigName);
  EigenState& st = make_state<EigenState>(e);
  st.H = p.history_size, st.M = p.embedded_dim;
  st.low = (float)p.threshold, st.high = 2 * st.low;  // params.LowThreshold() = threshold; params.HighThreshold() = 2*params.LowThreshold()
  st.L = (uint32_t)L, st.Lp = (uint32_t)((L + 3) & ~(size_t)3), st.chunks = (uint32_t)((L + bgs::kEigChunk - 1) / bgs::kEigChunk);
  const size_t H = (size_t)st.H, M = (size_t)st.M, Lp = st.Lp;
  // Nothing is initialised here: every buffer is written on the launch stream before it is read (see dmalloc).
  DMALLOC(st.hist, S * H * Lp);
  DMALLOC(st.avg, S * Lp * sizeof(float));
  DMALLOC(st.E, S * M * Lp * sizeof(float));
  DMALLOC(st.coeff, S * M * sizeof(float));
  DMALLOC(st.G, S * H * H * sizeof(unsigned long long));
  DMALLOC(st.W, S * M * H * sizeof(double));
  DMALLOC(st.lam, S * H * sizeof(double));
  DMALLOC(st.slab, S * st.chunks * M * sizeof(double));
  return BGS_OK;
}

// learning frames differ in their history slot, frame H builds the model, every later frame is the same launches
uint64_t eig_key(const bgs_engine* e, int i) { return (uint64_t)std::min<int64_t>(e->seen[i], eig_of(e).H + 1); }

bgs::EigenArgs eig_args(const bgs_engine* e, int first, const uint8_t* d_frames, uint8_t* d_fg, uint64_t* d_bits) {
  const EigenState& st = eig_of(e);
  const size_t f = (size_t)first, H = (size_t)st.H, M = (size_t)st.M, Lp = st.Lp;
  bgs::EigenArgs a{};
  a.cur = d_frames, a.fg = d_fg, a.bits = d_bits;
  a.hist = st.hist + f * H * Lp, a.avg = st.avg + f * Lp, a.E = st.E + f * M * Lp, a.G = st.G + f * H * H;
  a.W = st.W + f * M * H, a.lam = st.lam + f * H, a.slab = st.slab + f * st.chunks * M, a.coeff = st.coeff + f * M;
  a.n = (uint32_t)e->n, a.L = st.L, a.Lp = st.Lp, a.H = (uint32_t)st.H, a.M = (uint32_t)st.M, a.chunks = st.chunks;
  a.high = st.high;
  return a;
}

int eig_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t*, uint64_t* d_bits, hipStream_t s, uint32_t* flags) {
  const EigenState& st = eig_of(e);
  const bgs::EigenArgs a = eig_args(e, first, d_frames, d_fg, d_bits);
  const int64_t t = e->seen[first];  // the same for the whole run (eig_key), or all past H
  const unsigned per_elem = blocks_for(st.Lp), c = (unsigned)count;
  *flags = BGS_FG_VALID;  // the mask is written from frame 0 on; img_bgmodel never is
  if (t < st.H) {
    Timed tm(e, s, "eigen_store_kernel (history)");
    hipLaunchKernelGGL(bgs::eigen_store_kernel, dim3(per_elem, c), dim3(bgs::kBlock), 0, s, a, (uint32_t)t);
    return BGS_OK;
  }
  if (t == st.H) {  // cvCalcPCA, once per stream
    HIP_TRY(hipMemsetAsync(a.G, 0, (size_t)count * st.H * st.H * sizeof(unsigned long long), s));
    const unsigned gchunks = (st.Lp / 4 + bgs::kEigGramChunk - 1) / bgs::kEigGramChunk;
    hipLaunchKernelGGL(bgs::eigen_gram_kernel, dim3(gchunks, c), dim3(bgs::kBlock), 0, s, a);
    hipLaunchKernelGGL(bgs::eigen_solve_kernel, dim3(c), dim3(bgs::kWave), 0, s, a);
    hipLaunchKernelGGL(bgs::eigen_basis_kernel, dim3(per_elem, c), dim3(bgs::kBlock), 0, s, a);
  }
  Timed tm(e, s, "eigen_detect (project, coeff, reconstruct)");
  hipLaunchKernelGGL(bgs::eigen_project_kernel, dim3(st.chunks, c), dim3(bgs::kBlock), 0, s, a);
  hipLaunchKernelGGL(bgs::eigen_coeff_kernel, dim3(c), dim3(bgs::kBlock), 0, s, a);
  hipLaunchKernelGGL(bgs::eigen_reconstruct_kernel, dim3(blocks_for(e->n), c), dim3(bgs::kBlock), 0, s, a);
  return BGS_OK;
}

// bgs_get_state planes (include/bgs_hip.h)
int64_t eig_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  const EigenState& st = eig_of(e);
  const size_t H = (size_t)st.H, M = (size_t)st.M, L = st.L, Lp = st.Lp, k = (size_t)stream;
  const int64_t seen = e->seen[stream];
  if (!strcmp(plane, "count")) return copy_host(plane, dst, cap, &seen, 8);
  if (!strcmp(plane, "history")) {  // slots not yet filled read 0
    if (cap < H * L) return too_small(plane);
    std::memset(dst, 0, H * L);
    for (size_t t = 0; t < H && (int64_t)t < seen; ++t)
      if (fetch((uint8_t*)dst + t * L, st.hist + (k * H + t) * Lp, L)) return BGS_ERR_HIP;
    return (int64_t)(H * L);
  }
  const bool avg = !strcmp(plane, "avg"), val = !strcmp(plane, "eigenvalues"), vec = !strcmp(plane, "eigenvectors"), cf = !strcmp(plane, "coeff"), res = !strcmp(plane, "result");
  if (!avg && !val && !vec && !cf && !res) return unknown_plane(e, plane);
  if (seen <= (int64_t)H) return fail(BGS_ERR_STATE, "stream %d has no eigenbackground yet: it is built at frame %d", stream, st.H);
  if (avg) return copy_plane(plane, dst, cap, st.avg + k * Lp, L * 4);
  if (val) return copy_plane(plane, dst, cap, st.lam + k * H, H * 8);
  if (cf) return copy_plane(plane, dst, cap, st.coeff + k * M, M * 4);
  if (vec) {
    if (cap < M * L * 4) return too_small(plane);
    for (size_t i = 0; i < M; ++i)
      if (fetch((float*)dst + i * L, st.E + (k * M + i) * Lp, L * 4)) return BGS_ERR_HIP;
    return (int64_t)(M * L * 4);
  }
  // "result": not stored per frame; recomputed from avg, coeff and the eigenvectors by a launch of its own, after whatever the
  // caller's streams still hold
  if (cap < L * 4) return too_small(plane);
  DevPtr<float> r;
  DMALLOC(r, L * 4);
  HIP_TRY(hipDeviceSynchronize());
  bgs::EigenArgs a = eig_args(e, stream, nullptr, nullptr, nullptr);
  a.result = r;
  hipLaunchKernelGGL(bgs::eigen_reconstruct_kernel, dim3(blocks_for(e->n), 1), dim3(bgs::kBlock), 0, e->stream(), a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream()));
  return fetch(dst, r, L * 4) ? BGS_ERR_HIP : (int64_t)(L * 4);
}

// seen restarts at 0 (bgs_reset_stream): the history is refilled from slot 0 and the model rebuilt at frame H; nothing else to reset
constexpr Family kEigen = [] {
  Family f{};
  f.check_geometry = eig_check_geometry, f.allocate = eig_allocate, f.key = eig_key, f.run = eig_run, f.get_state = eig_get_state;
  return f;
}();
// frozen: the params object is filled once, on the first frame, and keeps what it was given (DPEigenbackgroundBGS.cpp `if(firstTime)`)
constexpr ParamBlock<bgs_eigen_params> kEigenBlock{&bgs_engine::eig, &kEigen, "bgs_eigen_params", kEigName, eig_defaults, eig_check, false};
