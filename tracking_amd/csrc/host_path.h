// host_path.h — the one staging lane of every entry point that takes a frame in host memory and hands results back to host memory
// (bgs_process, bgs_submit / bgs_wait, bgs_group_process, bgs_multicue_process, bgs_ingest_host); included inside
// bgs_hip.hip's anonymous namespace.  The rule all of them keep: a caller's pageable image never goes to hipMemcpy itself
// (d2h_staged's comment in bgs_hip.hip).  Rows are packed into / unpacked from page-locked images of the library's own (host_rows.h);
// only memory the caller asked to have page-locked in place (HostPath::pinned) is copied directly.  No kernel is named here.
#pragma once
#include "host_rows.h"

inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// One image, twice: page-locked on the host (h, unless !host) and on the device (d).  make() yields all that was asked for or nothing.
struct Staging {
  uint8_t *h = nullptr, *d = nullptr;
  Staging() = default;
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() { release(); }
  hipError_t make(size_t bytes, bool host = true, bool device = true) {  // 0 bytes: nothing to make
    hipError_t er = bytes && host ? hipHostMalloc((void**)&h, bytes, hipHostMallocDefault) : hipSuccess;
    if (bytes && device && er == hipSuccess) er = hipMalloc((void**)&d, bytes);
    if (er != hipSuccess) (void)hipGetLastError(), release();
    return er;
  }
  void release() {
    if (h) (void)hipHostFree(h), h = nullptr;
    if (d) (void)hipFree(d), d = nullptr;
  }
};

// `src` (rows x rb bytes, `step` from row to row, read through `map` if there is one) to device memory d_dst in `bands` bands on s,
// packed through st.h: the CPU packs band k+1 while band k is on the bus
inline hipError_t upload_rows(const Staging& st, uint8_t* d_dst, hipStream_t s, const uint8_t* src, size_t step, size_t rb, int rows, int bands, const RowMap* map = nullptr) {
  hipError_t er = hipSuccess;
  for (int b = 0; b < bands && er == hipSuccess; ++b) {
    const Band k = band_of(rows, bands, b);
    pack_rows(st.h, src, step, rb, k.y0, k.y1, map);
    er = hipMemcpyAsync(d_dst + (size_t)k.y0 * rb, st.h + (size_t)k.y0 * rb, (size_t)(k.y1 - k.y0) * rb, hipMemcpyHostToDevice, s);
  }
  return er;
}

// st.d to st.h in one copy on s; the caller unpacks st.h once s has got there (the lane's event, a stream synchronisation)
inline hipError_t download_whole(const Staging& st, size_t bytes, hipStream_t s) { return hipMemcpyAsync(st.h, st.d, bytes, hipMemcpyDeviceToHost, s); }

// A non-blocking HIP stream with the staging of one camera: input frame, mask, background (not copyable: its Staging members are
// not).  open() makes the stream alone - the engine's own stream is its synchronous lane's, and exists before there is staging -
// make() the rest, all or nothing.
struct Lane {
  hipStream_t hs = nullptr;
  hipEvent_t done = nullptr, band_ev[8] = {nullptr};  // done: null until make() has succeeded; band_ev: download_banded's, one per band, made when first used
  Staging in, fg, bg;
  ~Lane() { close(); }
  hipError_t open() { return hs ? hipSuccess : hipStreamCreateWithFlags(&hs, hipStreamNonBlocking); }
  hipError_t make(size_t in_bytes, size_t fg_bytes, size_t bg_bytes) {
    Staging* st[3] = {&in, &fg, &bg};
    const size_t bytes[3] = {in_bytes, fg_bytes, bg_bytes};
    hipError_t er = open();
    if (er == hipSuccess) er = hipEventCreateWithFlags(&done, hipEventDisableTiming);
    // the three host images first, then their device twins: the order bgs_submit has always allocated in (profiles/host_path_lane_ab.txt, last block)
    for (int part = 0; part < 2; ++part)
      for (int i = 0; i < 3 && er == hipSuccess; ++i) er = st[i]->make(bytes[i], part == 0, part == 1);
    if (er != hipSuccess) (void)hipGetLastError(), release_staging();
    return er;
  }
  void release_staging() {  // whatever of make() came to be; the stream stays
    if (hs) (void)hipStreamSynchronize(hs);
    in.release(), fg.release(), bg.release();
    if (done) (void)hipEventDestroy(done), done = nullptr;
    for (auto& ev : band_ev)
      if (ev) (void)hipEventDestroy(ev), ev = nullptr;
  }
  void close() {
    release_staging();
    if (hs) (void)hipStreamDestroy(hs), hs = nullptr;
  }
  struct Out { const Staging* st; uint8_t* dst; size_t step, rb; };  // one image on its way back: its staging and the caller's image (null: not wanted), rb bytes per row
  // a and b to staging in `bands` bands with an event behind each band, then band by band to the callers' images: band k is
  // unpacked while band k+1 is still on the bus
  hipError_t download_banded(int rows, int bands, const Out& a, const Out& b) {
    hipError_t er = hipSuccess;
    for (int i = 0; i < bands && er == hipSuccess; ++i) {
      const Band k = band_of(rows, bands, i);
      for (const Out* o : {&a, &b})
        if (o->dst && er == hipSuccess) er = hipMemcpyAsync(o->st->h + (size_t)k.y0 * o->rb, o->st->d + (size_t)k.y0 * o->rb, (size_t)(k.y1 - k.y0) * o->rb, hipMemcpyDeviceToHost, hs);
      if (er == hipSuccess && !band_ev[i]) er = hipEventCreateWithFlags(&band_ev[i], hipEventDisableTiming);
      if (er == hipSuccess) er = hipEventRecord(band_ev[i], hs);
    }
    for (int i = 0; i < bands && er == hipSuccess; ++i) {
      const Band k = band_of(rows, bands, i);
      er = hipEventSynchronize(band_ev[i]);
      for (const Out* o : {&a, &b})
        if (o->dst && er == hipSuccess) unpack_rows(o->dst, o->step, o->st->h, o->rb, k.y0, k.y1);
    }
    return er;
  }
};

// The host path of one engine: its lanes, the raw-frame staging of on-device ingest, the caller memory that is page-locked in place
// and the counters of bgs_get_state("hostpath").
struct HostPath {
  struct Pin { const void* ptr = nullptr; size_t bytes = 0; bool pinned = false, refused = false; };  // what the previous call passed in one role of one stream
  struct Submission {  // what bgs_wait needs of a stream's bgs_submit in flight
    bool pending = false, fg_direct = false, bg_direct = false;
    uint8_t *fg = nullptr, *bg = nullptr;  // the caller's output images
    size_t fg_step = 0, bg_step = 0;
    uint32_t flags = 0;
  };
  Lane sync;                // bgs_process; sync.hs is the engine's own stream (allocate)
  std::vector<Lane> lanes;  // bgs_submit / bgs_wait: one per camera, so that the uploads, kernels and downloads of different cameras overlap; made at a stream's first bgs_submit
  std::vector<Submission> sub;
  Staging raw, ingest_ws;   // ingest configurations that need device work: the raw frame, and bgs_ingest_device's workspace (device only)
  std::vector<Pin> pin;     // [stream][3]: 0 input, 1 mask, 2 background (every camera has its own buffers)
  std::vector<std::pair<const uint8_t*, size_t>> arenas;  // bgs_host_arena: caller memory page-locked as a whole; images inside it are DMA'd in place
  // diagnostics (bgs_get_state "hostpath"; bench.py host_path): what hipHostRegister cost and how often it ran, how long the CPU spent
  // copying images into / out of staging, bytes that crossed the bus each way
  double reg_ms = 0, stage_in_ms = 0, stage_out_ms = 0;
  int64_t reg_calls = 0, unreg_calls = 0, h2d_bytes = 0, d2h_bytes = 0, frames = 0;

  void set_streams(size_t n) { pin.assign(n * 3, Pin()), lanes = std::vector<Lane>(n), sub.assign(n, Submission()); }
  hipError_t timed_register(void* ptr, size_t bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t er = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    reg_ms += ms_since(t0), reg_calls++;
    if (er != hipSuccess) (void)hipGetLastError();
    return er;
  }
  // OpenCV's capture loop hands IBGS::process the SAME frame buffer every frame (VideoCapture.cpp:158-218: cvQueryFrame's image,
  // wrapped by cv::Mat img_input(frame)), and a caller that keeps its mask / background images allocated does the same on the way
  // out.  A buffer that comes back with the same address and size as in the previous call is page-locked (hipHostRegister, once)
  // and from then on the DMA engine reads / writes it directly: no staging copy by the CPU.  A different buffer in that role drops
  // the registration (after draining s, the stream that used it); release() drops them all.  Only contiguous images qualify (row
  // step = row bytes).  OPT-IN per role (`roles`: BGS_OPT_HOST_REGISTER): the engine cannot see a buffer being freed and another one
  // mapped at the same address, so the caller promises that a buffer it passes in an enabled role stays allocated until it passes a
  // different one or destroys the engine.
  bool pinned(int roles, int stream, int role, const void* ptr, size_t bytes, hipStream_t s) {
    if (!ptr || !bytes) return false;
    for (const auto& a : arenas)  // inside an arena the caller registered as a whole: nothing to do per image
      if ((const uint8_t*)ptr >= a.first && (const uint8_t*)ptr + bytes <= a.first + a.second) return true;
    if (!((roles >> role) & 1)) return false;
    Pin& p = pin[(size_t)stream * 3 + role];
    if (p.ptr == ptr && p.bytes == bytes) {
      if (p.pinned || p.refused) return p.pinned;
      if (timed_register(const_cast<void*>(ptr), bytes) == hipSuccess) return p.pinned = true;
      p.refused = true;  // not registrable (e.g. already registered by the caller, read-only mapping): keep staging
      return false;
    }
    if (p.pinned) {
      (void)hipStreamSynchronize(s);
      (void)hipHostUnregister(const_cast<void*>(p.ptr));
      unreg_calls++;
    }
    p = Pin();
    p.ptr = ptr, p.bytes = bytes;  // a candidate: registered when it comes back
    return false;
  }
  void unpin_roles_outside(int roles) {  // BGS_OPT_HOST_REGISTER changed: the roles no longer enabled go back to staging
    for (size_t i = 0; i < pin.size(); ++i)
      if (!((roles >> (i % 3)) & 1) && pin[i].pinned) (void)hipHostUnregister(const_cast<void*>(pin[i].ptr)), pin[i] = Pin();
  }
  void release() {  // free_all: the staging and the registrations go, the engine's own stream and the counters stay
    raw.release(), ingest_ws.release(), sync.release_staging();
    for (auto& ln : lanes) ln.close();
    unpin_roles_outside(0);
    pin.assign(pin.size(), Pin()), sub.assign(sub.size(), Submission());
    for (auto& a : arenas) (void)hipHostUnregister(const_cast<uint8_t*>(a.first));
    arenas.clear();
  }
};
