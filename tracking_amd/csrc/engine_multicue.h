// engine_multicue.h — host side of package_bgs/sjn SJN_MultiCueBGS: the model stage (kernel_multicue.h), the box stage
// (kernel_multicue_box.h, §5.14) and the whole-frame step that chains them as process() does; included inside bgs_hip.hip's anonymous
// namespace.
//
// What is here is the bgs_multicue object of include/bgs_hip.h: n_streams models, each with a frame counter of its own.  A stream is
// restarted alone (mc_reset_stream), any range of neighbouring streams is stepped in one call whatever their ages (mc_process_range), and
// mc_process_host steps one stream on a frame in host memory.  The IBGS class SJN_MultiCueBGS (tracking_amd/host/bgs_classes_multicue.inc)
// sits on a one-stream handle.  There is no bgs_algo for the class: BGS_ALGO_LAST, bgs_abi_version() and the type table stay as they are,
// and the class is reached as an IBGS and through FrameProcessor.  mc_defaults / mc_check / mc_check_geometry have the
// signatures a ParamBlock and a Family take.  Nothing here waits for the device except bgs_multicue_get_state and mc_process_host, and only
// the first mc_process_host call allocates.  The host-side state is not locked: calls on one handle from several host threads are not
// supported; disjoint ranges may be in flight on different HIP streams, since every plane and all scratch is indexed by stream.

constexpr const char* kMcName = "SJN_MultiCueBGS";

void mc_defaults(bgs_multicue_params* p) {  // the constructor, SJN_MultiCueBGS.cpp:30-48
  std::memset(p, 0, sizeof(*p));
  p->struct_size = (uint32_t)sizeof(*p);
  p->training_period = 20, p->t_model_threshold = 1, p->c_model_threshold = 10, p->learning_rate = 0.05f;
  p->texture_train_vol_range = 15, p->color_train_vol_range = 20, p->absorption_enable = 1, p->absorption_period = 200;
  p->reduced_width = 160, p->reduced_height = 120, p->back_clear_period = 300, p->cache_clear_period = 30;
}

// Needs no device.  nClearNum and the ranges are shorts in the reference, so the periods and ranges stop at 32767.
int mc_check(bgs_algo, const bgs_multicue_params& p) {
  if (!std::isfinite(p.learning_rate)) return fail(BGS_ERR_UNSUPPORTED, "%s: learning_rate must be finite", kMcName);
  const struct { const char* name; int v, lo; } lim[] = {{"training_period", p.training_period, 1}, {"absorption_period", p.absorption_period, 1},
      {"back_clear_period", p.back_clear_period, 1}, {"cache_clear_period", p.cache_clear_period, 1},
      {"texture_train_vol_range", p.texture_train_vol_range, 0}, {"color_train_vol_range", p.color_train_vol_range, 0}};
  for (const auto& l : lim)
    if (l.v < l.lo || l.v > 32767) return fail(BGS_ERR_UNSUPPORTED, "%s: %s %d is outside %d..32767 (a short in the reference)", kMcName, l.name, l.v, l.lo);
  if (p.reduced_width < 5 || p.reduced_height < 5)
    return fail(BGS_ERR_UNSUPPORTED, "%s: the reduced frame %d x %d has a side below 5 (no pixel with all six neighbours)", kMcName, p.reduced_width, p.reduced_height);
  if ((int64_t)p.reduced_width * p.reduced_height > BGS_CANNY_MAX_PIXELS)
    return fail(BGS_ERR_UNSUPPORTED, "%s: the reduced frame %d x %d is more than BGS_CANNY_MAX_PIXELS (%d) pixels (the per-box Canny runs on it)", kMcName, p.reduced_width,
                p.reduced_height, BGS_CANNY_MAX_PIXELS);
  return BGS_OK;
}
int mc_check_geometry(bgs_algo, int rows, int cols, int ch) {
  if (ch != 3) return fail(BGS_ERR_UNSUPPORTED, "%s: 3-channel frames only (ReduceImageSize, SJN_MultiCueBGS.cpp:547)", kMcName);
  if ((int64_t)rows * cols >= ((int64_t)1 << 31) / 3) return fail(BGS_ERR_UNSUPPORTED, "%s: a frame must stay below 2^31 bytes", kMcName);
  return BGS_OK;
}

struct McModel {
  int device = 0, S = 1;
  bgs_multicue_params p{};
  int rows = 0, cols = 0;  // of the frames; fixed by the first training call
  int rw = 0, rh = 0;
  size_t n = 0;
  std::vector<int64_t> count;  // g_iFrameCount, one per stream; 0: the stream's next frame initialises its model (mc_reset_kernel)
  bool have_landmark = false;  // of the piecewise calls, which need every stream at the same age: one flag serves them all
  Lane host;  // bgs_multicue_process: a HIP stream and the staging of one frame (in) and one image (fg), made by its first call (host_path.h)
  int taps[7] = {0};
  uint8_t* arena = nullptr;  // one allocation; everything below points into it
  uint8_t *red = nullptr, *gauss = nullptr, *xyz = nullptr, *landmark = nullptr;
  float* conf = nullptr;
  unsigned long long *overflow = nullptr, *box_overflow = nullptr;
  // the box stage's scratch (fore0, grey) and what the whole-frame step keeps between its launches
  uint8_t *fore0 = nullptr, *grey = nullptr, *s_landmark = nullptr, *s_fore = nullptr, *s_ghost = nullptr, *s_update = nullptr;
  int *s_count = nullptr, *s_boxes = nullptr;
  bgs::McPlanes tb{}, tc{}, cb{}, cc{};
  int16_t *tref = nullptr, *tcnt = nullptr, *cref = nullptr, *ccnt = nullptr;
  ~McModel() {
    host.close();  // drains its stream before the model goes
    if (arena) (void)hipFree(arena);
  }
};

int mc_allocate(McModel& m) {
  const size_t S = (size_t)m.S, n = m.n;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
  };
  struct Kind { bgs::McPlanes* pl; size_t K, NM, vsize; int cap; size_t head, mean, meta; };
  Kind kinds[4] = {{&m.tb, 6, 1, 4, bgs::kMcTSlots}, {&m.tc, 6, 1, 4, bgs::kMcTCacheSlots}, {&m.cb, 1, 3, 8, bgs::kMcCSlots}, {&m.cc, 1, 3, 8, bgs::kMcCCacheSlots}};
  // what has to start as 0 comes first (the heads: num = 0 makes every slot unread), then the referred indices (-1), then the rest
  for (Kind& k : kinds) k.head = take(S * k.K * 2 * n * 4);
  const size_t o_cnt = take(S * 7 * n * 2), o_over = take(8), o_bover = take(8), o_conf = take(S * n * 4), o_lm = take(S * n), zero_end = off;
  const size_t o_ref = take(S * 7 * n * 2), ref_end = off;
  for (Kind& k : kinds) k.mean = take(S * k.K * k.cap * k.NM * n * k.vsize), k.meta = take(S * k.K * k.cap * 3 * n * 4);
  const size_t o_red = take(S * n * 3), o_gauss = take(S * n * 3), o_xyz = take(S * n * 3);
  const size_t o_box = take(S * n * 6), o_cb = take(S * sizeof(int) * (1 + (size_t)bgs::kMcMaxBoxes * bgs::kMcBoxFields));
  HIP_TRY(hipMalloc((void**)&m.arena, off));
  HIP_TRY(hipMemset(m.arena, 0, zero_end));
  HIP_TRY(hipMemset(m.arena + o_ref, 0xff, ref_end - o_ref));  // int16 -1
  HIP_TRY(hipMemset(m.arena + o_red, 0, off - o_red));
  for (Kind& k : kinds) *k.pl = bgs::McPlanes{(int*)(m.arena + k.head), (void*)(m.arena + k.mean), (int*)(m.arena + k.meta), k.cap};
  m.tcnt = (int16_t*)(m.arena + o_cnt), m.ccnt = m.tcnt + S * 6 * n;
  m.tref = (int16_t*)(m.arena + o_ref), m.cref = m.tref + S * 6 * n;
  m.overflow = (unsigned long long*)(m.arena + o_over), m.conf = (float*)(m.arena + o_conf), m.landmark = m.arena + o_lm;
  m.red = m.arena + o_red, m.gauss = m.arena + o_gauss, m.xyz = m.arena + o_xyz;
  m.box_overflow = (unsigned long long*)(m.arena + o_bover);
  uint8_t* b = m.arena + o_box;
  m.fore0 = b, m.grey = b + S * n, m.s_landmark = b + 2 * S * n, m.s_fore = b + 3 * S * n, m.s_ghost = b + 4 * S * n, m.s_update = b + 5 * S * n;
  m.s_count = (int*)(m.arena + o_cb), m.s_boxes = m.s_count + S;
  return BGS_OK;
}

int mc_create(int device, int n_streams, const bgs_multicue_params* p, McModel* m) {
  m->device = device, m->S = n_streams, m->p = *p;
  m->rw = p->reduced_width, m->rh = p->reduced_height, m->n = (size_t)m->rw * m->rh;
  float cf[7];
  gaussian_kernel_f32(7, 0.7, cf);  // GaussianFiltering, :510-524
  for (int i = 0; i < 7; ++i) m->taps[i] = (int)std::lrintf(cf[i] * 256.f);
  m->count.assign((size_t)n_streams, 0);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(BGS_ERR_HIP, "no HIP device visible: libbgs_hip has no CPU path");
  HIP_TRY(hipSetDevice(device));
  int rc = mc_allocate(*m);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());  // the fills are done before the caller's stream sees the model
  return BGS_OK;
}

int mc_geometry(McModel& m, const char* fn, const void* d_frames, int rows, int cols, bool may_fix) {
  if (!d_frames || rows <= 0 || cols <= 0) return fail(BGS_ERR_INVALID, "%s: bad argument", fn);
  if (!m.rows && may_fix) {
    int rc = mc_check_geometry((bgs_algo)0, rows, cols, 3);
    if (rc) return rc;
    m.rows = rows, m.cols = cols;
  }
  if (rows != m.rows || cols != m.cols) return fail(BGS_ERR_GEOMETRY, "%s: %d x %d frames after %d x %d", fn, rows, cols, m.rows, m.cols);
  return BGS_OK;
}

// Every launch below covers streams [k, k + c) of the handle: the kernels index their planes by the stream's place in the launch, so each
// plane pointer is moved to stream k and d_frames, the maps and the outputs point at that stream's data.

// PreProcessing: reduce -> blur -> XYZ, three launches.  It does not depend on a stream's age, so a range of mixed ages shares them.
void mc_preprocess(McModel& m, int k, int c, const uint8_t* d_frames, hipStream_t s) {
  const unsigned S = (unsigned)c;
  const size_t at = (size_t)k * m.n * 3;
  hipLaunchKernelGGL(bgs::mc_reduce_kernel, dim3(blocks_for(m.n), S), dim3(bgs::kBlock), 0, s, d_frames, m.red + at, m.rows, m.cols, m.rh, m.rw,
                     (double)m.rows / (double)m.rh, (double)m.cols / (double)m.rw);
  bgs::BlurArgs b{};
  b.src = m.red + at, b.dst = m.gauss + at, b.rows = m.rh, b.cols = m.rw;
  for (int i = 0; i < 7; ++i) b.k[i] = m.taps[i];
  const dim3 tiles((unsigned)((m.rw + bgs::kBlurTW - 1) / bgs::kBlurTW), (unsigned)((m.rh + bgs::kBlurTH - 1) / bgs::kBlurTH), S);
  hipLaunchKernelGGL((bgs::ingest_blur7_kernel<3>), tiles, dim3(bgs::kBlock), 0, s, b);
  hipLaunchKernelGGL(bgs::mc_xyz_kernel, dim3(blocks_for((size_t)c * m.n)), dim3(bgs::kBlock), 0, s, (const uint8_t*)(m.gauss + at), m.xyz + at, (size_t)c * m.n);
}

// one kind of book from stream k on: K books a stream, NM means of vsize bytes a slot
bgs::McPlanes mc_planes_at(const bgs::McPlanes& pl, size_t K, size_t NM, size_t vsize, size_t k, size_t n) {
  return bgs::McPlanes{pl.head + k * K * 2 * n, (uint8_t*)pl.mean + k * K * (size_t)pl.cap * NM * n * vsize, pl.meta + k * K * (size_t)pl.cap * 3 * n, pl.cap};
}

bgs::McArgs mc_args(const McModel& m, int first) {
  bgs::McArgs a{};
  const size_t k = (size_t)first, n = m.n;
  a.xyz = m.xyz + k * n * 3, a.landmark = m.landmark + k * n;
  a.tb = mc_planes_at(m.tb, 6, 1, 4, k, n), a.tc = mc_planes_at(m.tc, 6, 1, 4, k, n), a.cb = mc_planes_at(m.cb, 1, 3, 8, k, n), a.cc = mc_planes_at(m.cc, 1, 3, 8, k, n);
  a.tref = m.tref + k * 6 * n, a.tcnt = m.tcnt + k * 6 * n, a.cref = m.cref + k * n, a.ccnt = m.ccnt + k * n, a.overflow = m.overflow;
  a.landmark_out = m.landmark + k * n, a.conf_out = m.conf + k * n;
  a.n = (uint32_t)m.n, a.rw = m.rw, a.rh = m.rh;
  a.rate = m.p.learning_rate, a.conf_thr = (float)m.p.t_model_threshold / 6.f;  // g_fConfidenceThre, :54
  a.trange = m.p.texture_train_vol_range, a.crange = m.p.color_train_vol_range;
  a.absorb = m.p.absorption_enable != 0, a.absorb_period = m.p.absorption_period, a.clear_period = m.p.back_clear_period;
  return a;
}

void mc_launch_update(const McModel& m, const bgs::McArgs& a, int c, hipStream_t s) {
  hipLaunchKernelGGL(bgs::mc_update_kernel, dim3(blocks_for(m.n), (unsigned)bgs::kMcBooks, (unsigned)c), dim3(bgs::kBlock), 0, s, a);
}

// The phase of a stream's next frame, which is what neighbouring streams must share to go into one launch (what Family::key is for engines)
enum McPhase { kMcTrain, kMcTrainLast, kMcDetect };
McPhase mc_phase(const McModel& m, int k) {
  const int64_t c = m.count[(size_t)k];
  return c < m.p.training_period ? kMcTrain : c == m.p.training_period ? kMcTrainLast : kMcDetect;
}
// the end of the run of streams that starts at k and ends before `end`, all in k's phase
int mc_run_end(const McModel& m, int k, int end) {
  int e = k + 1;
  while (e < end && mc_phase(m, e) == mc_phase(m, k)) ++e;
  return e;
}

// The piecewise calls work on every stream at once and keep one protocol state for all of them
int mc_lock_step(const McModel& m, const char* fn) {
  for (int k = 1; k < m.S; ++k)
    if (m.count[(size_t)k] != m.count[0])
      return fail(BGS_ERR_STATE, "%s: the streams are not all the same age (stream 0 has seen %lld frames, stream %d %lld): use bgs_multicue_process_range_device", fn,
                  (long long)m.count[0], k, (long long)m.count[(size_t)k]);
  return BGS_OK;
}

// BackgroundModeling_Par on the preprocessed frames of a run of training streams [k, e) in one phase.  Streams at frame 0 get their model
// initialised first, on the same HIP stream: one mc_reset_kernel launch per run of neighbours among them.
void mc_train_run(McModel& m, int k, int e, hipStream_t s) {
  for (int i = k; i < e;) {
    if (m.count[(size_t)i] != 0) {
      ++i;
      continue;
    }
    int j = i + 1;
    while (j < e && m.count[(size_t)j] == 0) ++j;
    hipLaunchKernelGGL(bgs::mc_reset_kernel, dim3(blocks_for(m.n), (unsigned)(j - i)), dim3(bgs::kBlock), 0, s, mc_args(m, i));
    i = j;
  }
  bgs::McArgs a = mc_args(m, k);
  const bool last = mc_phase(m, k) == kMcTrainLast;  // BackgroundModeling_Par's step 3, with nClearNum = training_period
  a.mode = last ? 1 : 0, a.clear_period = m.p.training_period;
  a.rate = m.p.learning_rate * 4;  // float
  mc_launch_update(m, a, e - k, s);
  for (int i = k; i < e; ++i) m.count[(size_t)i] += last ? 2 : 1;  // :308 and :87
}

void mc_landmark_run(McModel& m, int k, int e, uint8_t* d_landmark, float* d_conf, hipStream_t s) {
  bgs::McArgs a = mc_args(m, k);
  a.landmark_copy = d_landmark, a.conf_copy = d_conf;
  hipLaunchKernelGGL(bgs::mc_landmark_kernel, dim3(blocks_for(m.n), (unsigned)(e - k)), dim3(bgs::kBlock), 0, s, a);
}

void mc_update_run(McModel& m, int k, int e, const uint8_t* d_map, int ghost, hipStream_t s) {
  bgs::McArgs a = mc_args(m, k);
  a.map = d_map, a.mode = ghost ? 2 : 3;
  mc_launch_update(m, a, e - k, s);
}

int mc_train(McModel& m, const void* d_frames, int rows, int cols, hipStream_t s) {
  int rc = mc_lock_step(m, "bgs_multicue_train_device");
  if (rc || (rc = mc_geometry(m, "bgs_multicue_train_device", d_frames, rows, cols, true))) return rc;
  if (m.count[0] > m.p.training_period) return fail(BGS_ERR_STATE, "bgs_multicue_train_device: training is complete after %d frames", m.p.training_period + 1);
  HIP_TRY(hipSetDevice(m.device));
  mc_preprocess(m, 0, m.S, (const uint8_t*)d_frames, s);
  mc_train_run(m, 0, m.S, s);
  HIP_TRY(hipGetLastError());
  return BGS_OK;
}

int mc_landmark(McModel& m, const void* d_frames, int rows, int cols, void* d_landmark, void* d_conf, hipStream_t s) {
  if (!d_landmark) return fail(BGS_ERR_INVALID, "bgs_multicue_landmark_device: d_landmark is NULL");
  int rc = mc_lock_step(m, "bgs_multicue_landmark_device");
  if (rc) return rc;
  if (m.count[0] <= m.p.training_period) return fail(BGS_ERR_STATE, "bgs_multicue_landmark_device: training is not complete (%d frames)", m.p.training_period + 1);
  if ((rc = mc_geometry(m, "bgs_multicue_landmark_device", d_frames, rows, cols, false))) return rc;
  HIP_TRY(hipSetDevice(m.device));
  mc_preprocess(m, 0, m.S, (const uint8_t*)d_frames, s);
  mc_landmark_run(m, 0, m.S, (uint8_t*)d_landmark, (float*)d_conf, s);
  HIP_TRY(hipGetLastError());
  m.have_landmark = true;
  return BGS_OK;
}

int mc_update(McModel& m, const void* d_map, int ghost, hipStream_t s) {
  if (!d_map || (ghost != 0 && ghost != 1)) return fail(BGS_ERR_INVALID, "bgs_multicue_update_device: bad argument");
  int rc = mc_lock_step(m, "bgs_multicue_update_device");
  if (rc) return rc;
  if (!m.have_landmark) return fail(BGS_ERR_STATE, "bgs_multicue_update_device: no bgs_multicue_landmark_device call since the last update");
  HIP_TRY(hipSetDevice(m.device));
  mc_update_run(m, 0, m.S, (const uint8_t*)d_map, ghost, s);
  HIP_TRY(hipGetLastError());
  if (!ghost) m.have_landmark = false;
  return BGS_OK;
}

// PostProcessing and step 1 of UpdateModel_Par: three launches over streams [k, k + c) (kernel_multicue_box.h, compiled in bgs_multicue_box.hip).
// The caller's pointers are stream k's; the handle's own scratch is moved here.
void mc_launch_boxes(McModel& m, int k, int c, const uint8_t* d_landmark, const uint8_t* d_frames, uint8_t* d_fore, uint8_t* d_ghost, uint8_t* d_update, int* d_count,
                     int* d_boxes, hipStream_t s) {
  bgs::McBoxArgs a{};
  a.landmark = d_landmark, a.frames = d_frames, a.fore0 = m.fore0 + (size_t)k * m.n, a.grey = m.grey + (size_t)k * m.n, a.fore = d_fore, a.ghost = d_ghost, a.update = d_update;
  a.count = d_count, a.boxes = d_boxes, a.box_overflow = m.box_overflow;
  a.rows = m.rows, a.cols = m.cols, a.rw = m.rw, a.rh = m.rh;
  a.inv_fy = 1.0 / ((double)m.rh / (double)m.rows), a.inv_fx = 1.0 / ((double)m.rw / (double)m.cols);
  a.fh = (double)m.rows / (double)m.rh, a.fw = (double)m.cols / (double)m.rw;
  bgs::mc_box_launch(a, (unsigned)c, s);
}

int mc_boxes(McModel& m, const void* d_landmark, const void* d_frames, int rows, int cols, void* d_fore, void* d_ghost, void* d_update, void* d_count, void* d_boxes,
             hipStream_t s) {
  if (!d_landmark || !d_fore || !d_ghost || !d_update || !d_count || !d_boxes) return fail(BGS_ERR_INVALID, "bgs_multicue_boxes_device: NULL argument");
  int rc = mc_lock_step(m, "bgs_multicue_boxes_device");
  if (rc || (rc = mc_geometry(m, "bgs_multicue_boxes_device", d_frames, rows, cols, true))) return rc;
  HIP_TRY(hipSetDevice(m.device));
  mc_launch_boxes(m, 0, m.S, (const uint8_t*)d_landmark, (const uint8_t*)d_frames, (uint8_t*)d_fore, (uint8_t*)d_ghost, (uint8_t*)d_update, (int*)d_count, (int*)d_boxes, s);
  HIP_TRY(hipGetLastError());
  return BGS_OK;
}

// ingest_geom_kernel<1> over g.rows x g.cols pixels of `streams` images.  Defined at the end of bgs_hip.hip, behind bgs_ingest_device, so that
// the kernels of kernel_ingest.h are instantiated in the order they always were
void mc_launch_resize(const bgs::IngestArgs& g, unsigned streams, hipStream_t s);

// process(), SJN_MultiCueBGS.cpp:85-99: a training frame and zeros, or ForegroundExtraction, UpdateModel_Par and GetForegroundMap(result, NULL)
// for streams [first, first + count), which may be at different ages: the three PreProcessing launches once for the whole range, then every
// run of neighbours in one phase with one launch per kernel.  In lock step that is one run, and the launches are those of one stream.
int mc_process_range(McModel& m, const char* fn, int first, int count, const void* d_frames, int rows, int cols, void* d_out, hipStream_t s) {
  if (first < 0 || count < 1 || first > m.S - count) return fail(BGS_ERR_INVALID, "%s: streams %d..%d outside 0..%d", fn, first, first + count - 1, m.S - 1);
  if (!d_out) return fail(BGS_ERR_INVALID, "%s: d_out is NULL", fn);
  if (m.have_landmark) return fail(BGS_ERR_STATE, "%s: a bgs_multicue_landmark_device call is waiting for its updates", fn);
  int rc = mc_geometry(m, fn, d_frames, rows, cols, true);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(m.device));
  const size_t n = m.n, px = (size_t)rows * cols;
  const int end = first + count;
  mc_preprocess(m, first, count, (const uint8_t*)d_frames, s);
  for (int k = first, e; k < end; k = e) {
    e = mc_run_end(m, k, end);
    const uint8_t* frames = (const uint8_t*)d_frames + (size_t)(k - first) * px * 3;
    uint8_t* out = (uint8_t*)d_out + (size_t)(k - first) * px;
    if (mc_phase(m, k) != kMcDetect) {
      mc_train_run(m, k, e, s);
      HIP_TRY(hipMemsetAsync(out, 0, (size_t)(e - k) * px, s));
      continue;
    }
    uint8_t *lm = m.s_landmark + (size_t)k * n, *fore = m.s_fore + (size_t)k * n, *ghost = m.s_ghost + (size_t)k * n, *update = m.s_update + (size_t)k * n;
    mc_landmark_run(m, k, e, lm, nullptr, s);
    mc_launch_boxes(m, k, e - k, lm, frames, fore, ghost, update, m.s_count + k, m.s_boxes + (size_t)k * bgs::kMcMaxBoxes * bgs::kMcBoxFields, s);
    mc_update_run(m, k, e, ghost, 1, s);
    mc_update_run(m, k, e, update, 0, s);
    // cvResize(temp_image, return_image): the foreground map, bilinear, to the frame's size (kernel_ingest.h; the three channels are equal)
    bgs::IngestArgs g{};
    g.src = fore, g.dst = out, g.src_rows = m.rh, g.src_cols = m.rw, g.rw = cols, g.rh = rows, g.rows = rows, g.cols = cols, g.src_step = (size_t)m.rw;
    g.scale_x = 1. / ((double)cols / m.rw), g.scale_y = 1. / ((double)rows / m.rh);
    g.mode = (m.rw == 2 * cols && m.rh == 2 * rows) ? 2 : 1;
    mc_launch_resize(g, (unsigned)(e - k), s);
  }
  HIP_TRY(hipGetLastError());
  return BGS_OK;
}

// host-only: the stream's next frame is training frame 0, and until then bgs_multicue_get_state shows what a new handle shows
int mc_reset_stream(McModel& m, int stream) {
  if (stream < 0 || stream >= m.S) return fail(BGS_ERR_INVALID, "bgs_multicue_reset_stream: stream %d outside 0..%d", stream, m.S - 1);
  m.count[(size_t)stream] = 0;
  m.have_landmark = false;  // a piecewise landmark call that waited for its updates is dropped: its streams are no longer the same age, or all start again
  return BGS_OK;
}

// One stream, a frame in host memory, synchronous: upload, the range call for that stream, download of the one-channel image; the host
// writes out_channels equal channels.  The HIP stream and the staging are made here, by the first call: the geometry is known then.
int mc_process_host(McModel& m, int stream, const void* frame, int rows, int cols, size_t step, void* out, size_t out_step, int out_channels) {
  const char* fn = "bgs_multicue_process";
  if (!frame || !out || rows <= 0 || cols <= 0) return fail(BGS_ERR_INVALID, "%s: bad argument", fn);
  if (stream < 0 || stream >= m.S) return fail(BGS_ERR_INVALID, "%s: stream %d outside 0..%d", fn, stream, m.S - 1);
  if (out_channels != 1 && out_channels != 3) return fail(BGS_ERR_INVALID, "%s: out_channels must be 1 or 3", fn);
  const size_t row = (size_t)cols * 3, px = (size_t)rows * cols;
  if (step < row || out_step < (size_t)cols * out_channels)
    return fail(BGS_ERR_INVALID, "%s: row pitches %zu and %zu are below the row sizes %zu and %zu", fn, step, out_step, row, (size_t)cols * out_channels);
  int rc = mc_geometry(m, fn, frame, rows, cols, true);  // fixes the handle's geometry if nothing has yet: the staging below never changes size
  if (rc) return rc;
  HIP_TRY(hipSetDevice(m.device));
  Lane& ln = m.host;
  if (!ln.done) {
    const hipError_t er = ln.make(px * 3, px, 0);
    if (er != hipSuccess) return fail(BGS_ERR_HIP, "%s: staging buffers: %s", fn, hipGetErrorString(er));
  }
  HIP_TRY(upload_rows(ln.in, ln.in.d, ln.hs, (const uint8_t*)frame, step, row, rows, 1));
  if ((rc = mc_process_range(m, fn, stream, 1, ln.in.d, rows, cols, ln.fg.d, ln.hs))) return rc;
  HIP_TRY(download_whole(ln.fg, px, ln.hs));
  HIP_TRY(hipStreamSynchronize(ln.hs));
  if (out_channels == 1)
    unpack_rows((uint8_t*)out, out_step, ln.fg.h, (size_t)cols, 0, rows);
  else
    unpack_rows_gray3((uint8_t*)out, out_step, ln.fg.h, cols, 0, rows);
  return BGS_OK;
}

// one kind of book of one stream, transposed into the reference's order: book [nb][2], means [nb][cap][NM], meta [nb][cap][3]
// with nb = n * K books in (pixel, k) order; slots at and beyond m_iNumEntries read 0
template <class V>
int64_t mc_get_book(const McModel& m, const bgs::McPlanes& pl, size_t K, size_t NM, int stream, int what, const char* plane, void* dst, size_t cap) {
  const size_t n = m.n, C = (size_t)pl.cap, F = what == 0 ? 2 : what == 1 ? NM : 3;
  const size_t per = what == 0 ? 2 : C * F, esize = what == 1 ? sizeof(V) : 4, nb = n * K * per * esize;
  if (cap < nb) return too_small(plane);
  std::vector<int32_t> head(K * 2 * n);
  if (fetch(head.data(), pl.head + (size_t)stream * K * 2 * n, head.size() * 4)) return BGS_ERR_HIP;
  if (what == 0) {
    int32_t* o = (int32_t*)dst;
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < K; ++k) o[(i * K + k) * 2] = head[(k * 2) * n + i], o[(i * K + k) * 2 + 1] = head[(k * 2 + 1) * n + i];
    return (int64_t)nb;
  }
  std::memset(dst, 0, nb);
  std::vector<uint8_t> raw(K * C * F * n * esize);
  const uint8_t* src = what == 1 ? (const uint8_t*)pl.mean + (size_t)stream * raw.size() : (const uint8_t*)pl.meta + (size_t)stream * raw.size();
  if (fetch(raw.data(), src, raw.size())) return BGS_ERR_HIP;
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < K; ++k) {
      const size_t num = (size_t)std::min<int64_t>(std::max<int64_t>(head[(k * 2 + 1) * n + i], 0), (int64_t)C);
      for (size_t j = 0; j < num; ++j)
        for (size_t f = 0; f < F; ++f)
          std::memcpy((uint8_t*)dst + (((i * K + k) * C + j) * F + f) * esize, raw.data() + (((k * C + j) * F + f) * n + i) * esize, esize);
    }
  return (int64_t)nb;
}

int64_t mc_get_state(McModel& m, int stream, const char* plane, void* dst, size_t cap) {
  if (!plane || !dst) return fail(BGS_ERR_INVALID, "bgs_multicue_get_state: NULL argument");
  if (stream < 0 || stream >= m.S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, m.S - 1);
  HIP_TRY(hipSetDevice(m.device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t n = m.n, k = (size_t)stream;
  if (!strcmp(plane, "count")) return copy_host(plane, dst, cap, &m.count[k], 8);
  if (!strcmp(plane, "overflow")) return copy_plane(plane, dst, cap, m.overflow, 8);
  if (!strcmp(plane, "box_overflow")) return copy_plane(plane, dst, cap, m.box_overflow, 8);
  if (m.count[k] == 0) {
    // before its frame 0 a stream shows a new handle's planes whatever the device still holds of an earlier life (mc_reset_stream does not
    // touch the device): the referred indices -1, everything else 0
    const struct { const char* name; size_t bytes; int fill; } fresh[] = {
        {"gauss", n * 3, 0}, {"xyz", n * 3, 0}, {"conf", n * 4, 0}, {"landmark", n, 0}, {"tref", n * 12, 0xff}, {"tcnt", n * 12, 0}, {"cref", n * 2, 0xff}, {"ccnt", n * 2, 0},
        {"tbook", n * 48, 0}, {"tcache", n * 48, 0}, {"cbook", n * 8, 0}, {"ccache", n * 8, 0},
        {"tmeans", n * 6 * bgs::kMcTSlots * 4, 0}, {"tcache_means", n * 6 * bgs::kMcTCacheSlots * 4, 0}, {"tmeta", n * 6 * bgs::kMcTSlots * 12, 0},
        {"tcache_meta", n * 6 * bgs::kMcTCacheSlots * 12, 0}, {"cmeans", n * bgs::kMcCSlots * 24, 0}, {"ccache_means", n * bgs::kMcCCacheSlots * 24, 0},
        {"cmeta", n * bgs::kMcCSlots * 12, 0}, {"ccache_meta", n * bgs::kMcCCacheSlots * 12, 0}};
    for (const auto& f : fresh) {
      if (strcmp(plane, f.name)) continue;
      if (cap < f.bytes) return too_small(plane);
      std::memset(dst, f.fill, f.bytes);
      return (int64_t)f.bytes;
    }
    return fail(BGS_ERR_INVALID, "bgs_multicue_get_state: unknown plane %s", plane);
  }
  if (!strcmp(plane, "gauss")) return copy_plane(plane, dst, cap, m.gauss + k * n * 3, n * 3);
  if (!strcmp(plane, "xyz")) return copy_plane(plane, dst, cap, m.xyz + k * n * 3, n * 3);
  if (!strcmp(plane, "conf")) return copy_plane(plane, dst, cap, m.conf + k * n, n * 4);
  if (!strcmp(plane, "landmark")) return copy_plane(plane, dst, cap, m.landmark + k * n, n);
  if (!strcmp(plane, "cref")) return copy_plane(plane, dst, cap, m.cref + k * n, n * 2);
  if (!strcmp(plane, "ccnt")) return copy_plane(plane, dst, cap, m.ccnt + k * n, n * 2);
  if (!strcmp(plane, "tref") || !strcmp(plane, "tcnt")) {
    if (cap < n * 12) return too_small(plane);
    std::vector<int16_t> v(6 * n);
    if (fetch(v.data(), (plane[1] == 'r' ? m.tref : m.tcnt) + k * 6 * n, v.size() * 2)) return BGS_ERR_HIP;
    int16_t* o = (int16_t*)dst;
    for (size_t i = 0; i < n; ++i)
      for (size_t j = 0; j < 6; ++j) o[i * 6 + j] = v[j * n + i];
    return (int64_t)(n * 12);
  }
  const struct { const char* book; const char* means; const char* meta; const bgs::McPlanes* pl; bool colour; } kinds[] = {
      {"tbook", "tmeans", "tmeta", &m.tb, false}, {"tcache", "tcache_means", "tcache_meta", &m.tc, false},
      {"cbook", "cmeans", "cmeta", &m.cb, true}, {"ccache", "ccache_means", "ccache_meta", &m.cc, true}};
  for (const auto& kd : kinds) {
    const int what = !strcmp(plane, kd.book) ? 0 : !strcmp(plane, kd.means) ? 1 : !strcmp(plane, kd.meta) ? 2 : -1;
    if (what < 0) continue;
    return kd.colour ? mc_get_book<double>(m, *kd.pl, 1, 3, stream, what, plane, dst, cap) : mc_get_book<float>(m, *kd.pl, 6, 1, stream, what, plane, dst, cap);
  }
  return fail(BGS_ERR_INVALID, "bgs_multicue_get_state: unknown plane %s", plane);
}
