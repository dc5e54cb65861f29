// engine_group.h — bgs_group: several classes on the same frames (included by bgs_hip.hip).
//
// FrameProcessor::process hands ONE pre-processed frame to every enabled IBGS, one call after the other
// (FrameProcessor.cpp:169-340); BASELINE configs[2] is two of them on the same 3840x2160 frames.  A group runs the byte-stream
// classes among them (FrameDifference, StaticFrameDifference, WeightedMovingMean, WeightedMovingVariance,
// AdaptiveBackgroundLearning, SigmaDelta - at most one instance of each) as ONE kernel over one read of the frame and one
// shared history ring (kernel_fanout.h); every other class (and a second instance of a fused one) is a member engine fed the
// same device frame.  Outputs, warm-up conventions and states are those of the separate engines, bit for bit: the state of a fused
// class IS its family's state struct (engine_pointwise.h), the ring the FrameHistory an engine has, and what acts on them (ABL's rule
// and table, first frames, planes, geometry refusals, the persistent grid, the timer) the functions the engines call.
// The streams of a group advance in lock-step (whole-batch calls); the host entry point serves single-stream groups, which is
// what FrameProcessor is.
#pragma once
#include "kernel_fanout.h"

struct bgs_group {
  int device = 0, S = 1, rows = 0, cols = 0, ch = 0;
  size_t n = 0;
  std::vector<bgs_algo> algos;
  std::vector<bgs_params> params;
  std::vector<unsigned> fan_bit;        // per class: its kFan* bit, 0 = member engine
  std::vector<bgs_engine*> member;      // per class: own engine, or null when fused
  unsigned fused = 0;                   // union of the fan bits
  FrameHistory hist;                    // ONE ring of 2 (FD alone) or 3 slots for all of them, at position `seen`: a group has no bgs_reset_stream
  SbgState sfd, abl;                    // abl.lut follows params lazily: it is rebuilt by the next process call after bgs_group_set_params
  SdState sd;
  int64_t seen = 0, abl_counter = 0;    // ONE ABL counter for all the streams
  int n_cu = 256;
  hipStream_t stream = nullptr;
  // bgs_group_process (single-stream groups): staging of the frame and of every class's mask and background (host_path.h), made
  // whole by the first call and released with the group
  Staging in;
  std::vector<Staging> fg, bg;
  LaunchTimer timer;                    // of the fused launch
};

namespace {

unsigned fan_bit_of(bgs_algo a) {
  switch (a) {
    case BGS_FRAME_DIFF: return bgs::kFanFD;
    case BGS_STATIC_FRAME_DIFF: return bgs::kFanSFD;
    case BGS_WMM: return bgs::kFanWMM;
    case BGS_WMV: return bgs::kFanWMV;
    case BGS_ABL: return bgs::kFanABL;
    case BGS_SIGMA_DELTA: return bgs::kFanSD;
    default: return 0;
  }
}

int group_index_of(const bgs_group* g, unsigned bit) {
  for (size_t i = 0; i < g->fan_bit.size(); ++i)
    if (g->fan_bit[i] == bit) return (int)i;
  return -1;
}

int group_build_lut(bgs_group* g) {
  const int i = group_index_of(g, bgs::kFanABL);
  return i < 0 ? BGS_OK : abl_table(g->abl, g->params[i].alpha, g->device, g->stream);
}

int group_allocate(bgs_group* g, int rows, int cols, int ch) {
  int rc = check_geometry((g->fused & bgs::kFanSD) ? &kSigmaDelta : nullptr, BGS_SIGMA_DELTA, rows, cols, ch);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(g->device));
  g->rows = rows, g->cols = cols, g->ch = ch, g->n = (size_t)rows * cols;
  const size_t fb = g->n * g->S * ch;
  if (!g->stream) HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
  g->hist.nring = (g->fused & (bgs::kFanWMM | bgs::kFanWMV)) ? 3 : (g->fused & bgs::kFanFD) ? 2 : 0;
  for (int i = 0; i < g->hist.nring; ++i) HIP_TRY(hipMalloc((void**)&g->hist.slot[i].p, fb));
  if (g->fused & bgs::kFanSFD) HIP_TRY(hipMalloc((void**)&g->sfd.bg.p, fb));
  if (g->fused & bgs::kFanABL) HIP_TRY(hipMalloc((void**)&g->abl.bg.p, fb));
  if (g->fused & bgs::kFanSD) {
    HIP_TRY(hipMalloc((void**)&g->sd.mt.p, fb));
    HIP_TRY(hipMalloc((void**)&g->sd.vt.p, fb));
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, g->device) == hipSuccess && prop.multiProcessorCount > 0) g->n_cu = prop.multiProcessorCount;
  rc = group_build_lut(g);
  if (rc) return rc;
  for (size_t i = 0; i < g->member.size(); ++i)
    if (g->member[i]) {
      rc = bgs_set_geometry(g->member[i], rows, cols, ch);
      if (rc) return rc;
    }
  return BGS_OK;
}

template <int G, int C>
void group_launch_fan(bgs_group* g, const bgs::FanArgs& a, hipStream_t s) {
  if ((a.mask & bgs::kFanABL) && a.abl_update) {  // the table form is persistent, like abl_kernel
    const size_t per_tile = (size_t)bgs::kAblBlock * G, ntiles = (a.npix + per_tile - 1) / per_tile;
    hipLaunchKernelGGL((bgs::fan_kernel<G, C, true>), (resident_grid<bgs::fan_kernel<G, C, true>>(ntiles, g->n_cu)), dim3(bgs::kAblBlock), 0, s, a, (const uint8_t*)g->abl.lut.p);
  } else {
    hipLaunchKernelGGL((bgs::fan_kernel<G, C, false>), dim3(blocks_for((a.npix + G - 1) / G)), dim3(bgs::kBlock), 0, s, a, (const uint8_t*)nullptr);
  }
}

// One frame of every stream for every class; device pointers, asynchronous on s.
int group_process_device(bgs_group* g, const uint8_t* d_frames, uint8_t* const* d_fg, uint8_t* const* d_bg, hipStream_t s, uint32_t* out_flags) {
  const int K = (int)g->algos.size();
  if (out_flags)
    for (int i = 0; i < K; ++i) out_flags[i] = 0;
  if (!g->n) return fail(BGS_ERR_INVALID, "geometry not set: call bgs_group_set_geometry or bgs_group_process first");
  if (!d_frames) return fail(BGS_ERR_INVALID, "d_frames is NULL");
  HIP_TRY(hipSetDevice(g->device));
  const int C = g->ch;
  const size_t npix = g->n * g->S, fb = npix * C;
  const int64_t t = g->seen;
  std::vector<uint32_t> flags((size_t)K, 0);
  if (g->fused) {
    int rc = group_build_lut(g);  // alpha may have changed through bgs_group_set_params
    if (rc) return rc;
    bgs::FanArgs a{};
    a.npix = npix;
    FrameHistory::Frames f;
    HIP_TRY(g->hist.resolve(t, t, 0, fb, d_frames, s, &f));
    a.cur = f.cur, a.p1 = f.h1, a.p2 = f.h2;
    auto out_of = [&](unsigned bit, bgs::FanOut& o, bool with_bg, uint32_t fl) -> const bgs_params& {  // class `bit` takes part in this launch
      const int i = group_index_of(g, bit);
      const bgs_params& p = g->params[i];
      o.fg = d_fg ? d_fg[i] : nullptr, o.bg = (with_bg && d_bg) ? d_bg[i] : nullptr, o.bits = nullptr;
      o.thr = p.threshold, o.enable_thr = p.enable_threshold, o.enable_weight = p.enable_weight;
      a.mask |= bit, flags[i] = fl;
      return p;
    };
    if ((g->fused & bgs::kFanFD) && t >= 1) out_of(bgs::kFanFD, a.fd, false, BGS_FG_VALID);
    if (g->fused & bgs::kFanSFD) {
      out_of(bgs::kFanSFD, a.sfd, false, BGS_FG_VALID | BGS_BG_VALID);
      uint8_t* bg = d_bg ? d_bg[group_index_of(g, bgs::kFanSFD)] : nullptr;
      HIP_TRY(sbg_first_frame(g->sfd, t, 0, d_frames, fb, s));
      a.sfd_bg = g->sfd.bg;
      if (bg) HIP_TRY(hipMemcpyAsync(bg, a.sfd_bg, fb, hipMemcpyDeviceToDevice, s));
    }
    if ((g->fused & bgs::kFanWMM) && t >= 2) out_of(bgs::kFanWMM, a.wmm, true, BGS_FG_VALID | BGS_BG_VALID);
    if ((g->fused & bgs::kFanWMV) && t >= 2) out_of(bgs::kFanWMV, a.wmv, false, BGS_FG_VALID);
    if (g->fused & bgs::kFanABL) {
      const bgs_params& p = out_of(bgs::kFanABL, a.abl, true, BGS_FG_VALID | BGS_BG_VALID);
      HIP_TRY(sbg_first_frame(g->abl, t, 0, d_frames, fb, s));
      a.abl_state = g->abl.bg, a.abl_update = abl_updates(p, g->abl_counter);
      abl_count(p, g->abl_counter);
    }
    if (g->fused & bgs::kFanSD) {
      const bgs_params& p = g->params[group_index_of(g, bgs::kFanSD)];
      if (t == 0 && (rc = sd_first_frame(g->sd, 0, d_frames, fb, g->cols, p, s))) return rc;
      if (t >= 1) out_of(bgs::kFanSD, a.sd, false, BGS_FG_VALID);
      a.sd_mt = g->sd.mt, a.sd_vt = g->sd.vt, a.sd_N = (uint32_t)p.sd_amp_factor, a.sd_vmin = (uint8_t)p.sd_min_var, a.sd_vmax = (uint8_t)p.sd_max_var;
    }
    if (a.mask) {
      const void* ptrs[] = {a.cur, a.p1, a.p2, a.fd.fg, a.sfd.fg, a.wmm.fg, a.wmm.bg, a.wmv.fg, a.abl.fg, a.abl.bg, a.sd.fg};
      int G = npix % 4 ? 1 : 4;
      for (const void* q : ptrs)
        if (q && !aligned(q, 4)) G = 1;
      {
        Timed tm(g->timer, s);
        if (C == 3 && G == 4) group_launch_fan<4, 3>(g, a, s);
        else if (C == 3) group_launch_fan<1, 3>(g, a, s);
        else if (G == 4) group_launch_fan<4, 1>(g, a, s);
        else group_launch_fan<1, 1>(g, a, s);
      }
      HIP_TRY(hipGetLastError());
    }
  }
  for (int i = 0; i < K; ++i)
    if (g->member[i]) {
      int rc = process_range(g->member[i], 0, g->S, d_frames, d_fg ? d_fg[i] : nullptr, d_bg ? d_bg[i] : nullptr, nullptr, s, &flags[i]);
      if (rc) return rc;
    }
  g->seen++;
  if (out_flags)
    for (int i = 0; i < K; ++i) out_flags[i] = flags[i];
  return BGS_OK;
}

}  // namespace

extern "C" {

int bgs_group_create(const bgs_algo* algos, const bgs_params* const* params, int n_algos, int hip_device, int n_streams, bgs_group** out) {
  if (!algos || !out || n_algos < 1 || n_algos > 64) return fail(BGS_ERR_INVALID, "bgs_group_create: bad argument");
  if (n_streams < 1) return fail(BGS_ERR_INVALID, "n_streams must be >= 1");
  *out = nullptr;
  bgs_group* g = new bgs_group();
  g->device = hip_device, g->S = n_streams;
  for (int i = 0; i < n_algos; ++i) {
    bgs_params p;
    std::memset(&p, 0, sizeof(p));
    p.struct_size = sizeof(p);
    int rc = bgs_default_params(algos[i], &p);
    if (!rc && params && params[i]) {
      if (params[i]->struct_size != sizeof(bgs_params)) rc = fail(BGS_ERR_INVALID, "bgs_params.struct_size mismatch (class %d)", i);
      else p = *params[i];
    }
    if (!rc && algos[i] == BGS_VUMETER) rc = fail(BGS_ERR_UNSUPPORTED, "VuMeter is not built for class groups (its background image is gray)");
    if (!rc)  // a class with a parameter block of its own: a group carries bgs_params only
      for_each_block([&](const auto& b) {
        if (family_of(algos[i]) == b.fam) rc = fail(BGS_ERR_UNSUPPORTED, "%s is not built for class groups (its parameters are %s, not bgs_params)", b.class_name, b.struct_name);
      });
    unsigned bit = fan_bit_of(algos[i]);
    if (bit & g->fused) bit = 0;  // a second instance of a fused class runs as a member engine
    bgs_engine* m = nullptr;
    if (!rc && !bit) rc = bgs_create(algos[i], &p, hip_device, n_streams, &m);
    if (rc) {
      for (bgs_engine* e : g->member)
        if (e) bgs_destroy(e);
      delete g;
      return rc;
    }
    g->algos.push_back(algos[i]), g->params.push_back(p), g->fan_bit.push_back(bit), g->member.push_back(m);
    g->fused |= bit;
  }
  if (g->fused) {  // no CPU path, like bgs_create
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || hip_device < 0 || hip_device >= ndev) {
      delete g;
      return fail(BGS_ERR_HIP, "no HIP device visible: libbgs_hip has no CPU path");
    }
  }
  g->fg = std::vector<Staging>((size_t)n_algos), g->bg = std::vector<Staging>((size_t)n_algos);
  *out = g;
  return BGS_OK;
}

void bgs_group_destroy(bgs_group* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  (void)hipDeviceSynchronize();
  for (bgs_engine* e : g->member)
    if (e) bgs_destroy(e);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  delete g;  // the states, the ring, the timer and the staging release themselves
}

int bgs_group_size(const bgs_group* g) { return g ? (int)g->algos.size() : BGS_ERR_INVALID; }

/* 1 when class `index` runs inside the fused kernel, 0 when it is a member engine */
int bgs_group_is_fused(const bgs_group* g, int index) {
  if (!g || index < 0 || index >= (int)g->algos.size()) return BGS_ERR_INVALID;
  return g->fan_bit[index] != 0;
}

int bgs_group_set_params(bgs_group* g, int index, const bgs_params* params) {
  if (!g || !params) return fail(BGS_ERR_INVALID, "NULL argument");
  if (index < 0 || index >= (int)g->algos.size()) return fail(BGS_ERR_INVALID, "class %d outside 0..%d", index, (int)g->algos.size() - 1);
  if (params->struct_size != sizeof(bgs_params)) return fail(BGS_ERR_INVALID, "bgs_params.struct_size mismatch");
  if (g->member[index]) return bgs_set_params(g->member[index], params);
  g->params[index] = *params;
  return BGS_OK;
}

int bgs_group_set_option(bgs_group* g, int option, int64_t value) {
  if (!g) return fail(BGS_ERR_INVALID, "group is NULL");
  if (option == BGS_OPT_BORROW_FRAMES) {
    g->hist.mode = value ? FrameHistory::kBorrowed : FrameHistory::kPrivate;
    for (bgs_engine* e : g->member)
      if (e && (e->algo == BGS_FRAME_DIFF || e->algo == BGS_WMM || e->algo == BGS_WMV)) (void)bgs_set_option(e, option, value);
    return BGS_OK;
  }
  for (bgs_engine* e : g->member)
    if (e) (void)bgs_set_option(e, option, value);
  return BGS_OK;
}

int bgs_group_set_geometry(bgs_group* g, int rows, int cols, int channels) {
  if (!g) return fail(BGS_ERR_INVALID, "group is NULL");
  if (g->n) {
    if (rows == g->rows && cols == g->cols && channels == g->ch) return BGS_OK;
    return fail(BGS_ERR_GEOMETRY, "a group keeps its geometry (%dx%dx%d); create a new one for %dx%dx%d", g->rows, g->cols, g->ch, rows, cols, channels);
  }
  int rc = group_allocate(g, rows, cols, channels);
  if (rc) g->hist.release(), g->sfd = SbgState(), g->abl = SbgState(), g->sd = SdState(), g->n = 0;  // everything, whatever part of it came to be
  return rc;
}

int bgs_group_process_batch_device(bgs_group* g, const void* d_frames, void* const* d_fg, void* const* d_bg, void* hip_stream, uint32_t* out_flags) {
  if (!g) return fail(BGS_ERR_INVALID, "group is NULL");
  return group_process_device(g, (const uint8_t*)d_frames, (uint8_t* const*)d_fg, (uint8_t* const*)d_bg, (hipStream_t)hip_stream, out_flags);
}

int bgs_group_process(bgs_group* g, const uint8_t* in, int rows, int cols, int channels, size_t in_step, uint8_t* const* fg, const size_t* fg_step,
                      uint8_t* const* bg, const size_t* bg_step, uint32_t* out_flags) {
  if (!g) return fail(BGS_ERR_INVALID, "group is NULL");
  const int K = (int)g->algos.size();
  if (out_flags)
    for (int i = 0; i < K; ++i) out_flags[i] = 0;
  if (g->S != 1) return fail(BGS_ERR_INVALID, "bgs_group_process serves single-stream groups (this one has %d streams): use bgs_group_process_batch_device", g->S);
  if (!in || rows <= 0 || cols <= 0) return BGS_OK;  // if(img_input.empty()) return;
  if (channels != 1 && channels != 3) return fail(BGS_ERR_UNSUPPORTED, "channels must be 1 or 3");
  if (in_step < (size_t)cols * channels) return fail(BGS_ERR_INVALID, "in_step %zu < cols*channels", in_step);
  int rc = bgs_group_set_geometry(g, rows, cols, channels);
  if (rc) return rc;
  const size_t fb = g->n * channels, row = (size_t)cols * channels;
  auto bg_row = [&](int i) { return (size_t)cols * (g->algos[i] == BGS_ASBL ? 1 : channels); };  // bytes of a row of class i's background
  if (!g->in.h) {
    // all or nothing: a staging set with some class's buffers missing would silently drop that class's outputs
    hipError_t er = g->in.make(fb);
    for (int i = 0; i < K && er == hipSuccess; ++i)
      if ((er = g->fg[i].make(g->n)) == hipSuccess) er = g->bg[i].make(bg_row(i) * rows);
    if (er != hipSuccess) {
      g->in.release();
      for (int i = 0; i < K; ++i) g->fg[i].release(), g->bg[i].release();
      return fail(BGS_ERR_HIP, "bgs_group_process: staging buffers: %s", hipGetErrorString(er));
    }
  }
  HIP_TRY(upload_rows(g->in, g->in.d, g->stream, in, in_step, row, rows, 1));  // ONE upload for all the classes
  std::vector<uint8_t*> dfg((size_t)K), dbg((size_t)K);
  for (int i = 0; i < K; ++i) dfg[i] = (fg && fg[i]) ? g->fg[i].d : nullptr, dbg[i] = (bg && bg[i]) ? g->bg[i].d : nullptr;
  std::vector<uint32_t> flags((size_t)K, 0);
  {
    FrameHistory::Scope own(g->hist);  // the staging buffer is reused every frame: private history, whatever BGS_OPT_BORROW_FRAMES says
    rc = group_process_device(g, g->in.d, dfg.data(), dbg.data(), g->stream, flags.data());
  }
  if (rc) return rc;
  for (int i = 0; i < K; ++i) {
    if (!(flags[i] & BGS_FG_VALID)) dfg[i] = nullptr;  // from here on: what comes back
    if (!(flags[i] & BGS_BG_VALID)) dbg[i] = nullptr;
    if (dfg[i]) HIP_TRY(download_whole(g->fg[i], g->n, g->stream));
    if (dbg[i]) HIP_TRY(download_whole(g->bg[i], bg_row(i) * rows, g->stream));
  }
  HIP_TRY(hipStreamSynchronize(g->stream));
  for (int i = 0; i < K; ++i) {
    if (dfg[i]) unpack_rows(fg[i], fg_step ? fg_step[i] : (size_t)cols, g->fg[i].h, (size_t)cols, 0, rows);
    if (dbg[i]) unpack_rows(bg[i], bg_step ? bg_step[i] : bg_row(i), g->bg[i].h, bg_row(i), 0, rows);
  }
  if (out_flags)
    for (int i = 0; i < K; ++i) out_flags[i] = flags[i];
  return BGS_OK;
}

int64_t bgs_group_get_state(bgs_group* g, int index, int stream, const char* plane, void* dst, size_t cap) {
  if (!g || !plane || !dst) return fail(BGS_ERR_INVALID, "NULL argument");
  if (index < 0 || index >= (int)g->algos.size()) return fail(BGS_ERR_INVALID, "class %d outside 0..%d", index, (int)g->algos.size() - 1);
  if (g->member[index]) return bgs_get_state(g->member[index], stream, plane, dst, cap);
  if (!g->n) return fail(BGS_ERR_STATE, "no model yet");
  if (stream < 0 || stream >= g->S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, g->S - 1);
  if (hipSetDevice(g->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(BGS_ERR_HIP, "device sync failed");
  const size_t nb = g->n * g->ch;
  const uint8_t* src = nullptr;
  const int64_t t = g->seen;
  switch (g->fan_bit[index]) {  // the planes of the class's family; a fused SigmaDelta answers mt / vt only, not the engine's "bg"
    case bgs::kFanSFD: src = sbg_plane(g->sfd, t, nb, stream, plane); break;
    case bgs::kFanABL: src = sbg_plane(g->abl, t, nb, stream, plane); break;
    case bgs::kFanSD: src = sd_plane(g->sd, t, nb, stream, plane); break;
    default: src = g->hist.mode == FrameHistory::kBorrowed ? nullptr : g->hist.plane(t, t, plane, nb * stream);  // lent history: the ring holds nothing
  }
  if (!src) return fail(BGS_ERR_STATE, "unknown state plane '%s' for class %d of the group", plane, index);
  return copy_plane(plane, dst, cap, src, nb);
}

int64_t bgs_group_frames_seen(const bgs_group* g) { return g ? g->seen : BGS_ERR_INVALID; }

int bgs_group_enable_kernel_timing(bgs_group* g, int on) {
  if (!g) return fail(BGS_ERR_INVALID, "group is NULL");
  g->timer.enable(on != 0);
  return BGS_OK;
}

/* mean duration in ms of the fused launches since timing was enabled (the device is drained first) */
int bgs_group_kernel_timing(bgs_group* g, double* avg_ms, int64_t* launches) {
  if (!g || !avg_ms || !launches) return fail(BGS_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(g->device));
  HIP_TRY(hipDeviceSynchronize());
  double total = 0;
  (void)g->timer.read(false, INT64_MAX, nullptr, launches, &total);
  *avg_ms = *launches ? total / (double)*launches : 0.0;
  return BGS_OK;
}

}  // extern "C"
