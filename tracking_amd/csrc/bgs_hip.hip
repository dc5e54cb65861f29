// bgs_hip.hip — the C ABI of libbgs_hip (include/bgs_hip.h) and the engine behind it.
//
// The engine is the device-side twin of one reference IBGS object per stream: it owns the model state of
// n_streams independent streams as SoA planes in HBM and turns every IBGS::process call
// (package_bgs/IBGS.h:24) into ONE fused kernel launch.  Host entry points stage through pinned memory;
// device entry points take HBM pointers and launch over streams x pixels.  There is no CPU fallback: if HIP
// is unavailable every compute entry point fails with BGS_ERR_HIP.
//
// This file holds what every class shares: the engine's generic members, allocation helpers (DevPtr, DMALLOC, model_allocate), the
// split of a call into runs of streams (launch_key), the packed-mask plumbing, clip calls, the host path and the C entry points.
// What a class is and does lives in its engine_*.h: its state struct (a FamilyState: device buffers, tables, per-stream counters;
// the engine holds it as `model`) and its checks, model allocation, launch key, one frame, fused clip and state export, reached
// only through that file's `Family` of entry points, looked up once per engine by family_of() below.
#include "../../include/bgs_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <atomic>
#include <vector>

#include "kernel_gmg.h"
#include "kernel_ingest.h"
#include "kernel_kde.h"
#include "kernel_dp2.h"
#include "kernel_lb.h"
#include "kernel_vumeter.h"
#include "kernel_fuzzy.h"
#include "kernel_t2f.h"
#include "kernel_eigen.h"
#include "kernel_imbs.h"
#include "kernel_multilayer.h"
#include "kernel_canny.h"
#include "gridcut.h"
#include "kernel_multicue.h"
#include "multicue_box.h"
#include "kernel_cc.h"
#include "kernel_dp.h"
#include "kernel_mog1.h"
#include "kernel_mog2.h"
#include "kernel_pointwise.h"
#include "kernel_stencil.h"
#include "kernel_subsense.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                           \
  do {                                                                                          \
    hipError_t e__ = (expr);                                                                    \
    if (e__ != hipSuccess) return fail(BGS_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
  } while (0)

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// Device -> pageable host memory (bgs_get_state, the blob lists): through a page-locked bounce buffer of the library's own, never
// hipMemcpy straight into the caller's memory.  For copies past a size threshold the HIP runtime page-locks the caller's buffer on the
// fly and KEEPS the last eight such mappings, looked up by host ADDRESS (ROCclr: hsaCopyStagedOrPinned -> pinHostMemory / addPinnedMem
// / findPinnedMem).  A caller that frees such a buffer and gets the same address back from the next allocation - numpy does, for every
// array past malloc's mmap threshold - is served the stale mapping, and the copy engine then writes through pages that are gone:
// round 4's GPU suite died twice that way (rocr::core::Runtime::VMFaultHandler -> abort while a test read a model plane back,
// profiles/r04_vmfault_backtrace.txt), in different tests, with no kernel of this library running.  A page-locked destination takes
// the direct path.  One buffer per process, serialised: these are diagnostics and small result lists, not the frame path (bgs_process
// stages through the engine's own page-locked images).
int d2h_staged(void* dst, const void* src, size_t bytes) {
  static std::mutex mu;
  static uint8_t* bounce = nullptr;
  constexpr size_t kBounce = (size_t)4 << 20;
  std::lock_guard<std::mutex> lk(mu);
  if (!bounce && hipHostMalloc((void**)&bounce, kBounce, hipHostMallocPortable) != hipSuccess) {
    bounce = nullptr;
    return fail(BGS_ERR_HIP, "hipHostMalloc of the read-back buffer failed");
  }
  for (size_t o = 0; o < bytes; o += kBounce) {
    const size_t n = std::min(kBounce, bytes - o);
    if (hipMemcpy(bounce, (const uint8_t*)src + o, n, hipMemcpyDeviceToHost) != hipSuccess) return fail(BGS_ERR_HIP, "hipMemcpy (device to host) failed");
    std::memcpy((uint8_t*)dst + o, bounce, n);
  }
  return BGS_OK;
}
inline unsigned blocks_for(size_t groups) { return (unsigned)((groups + bgs::kBlock - 1) / bgs::kBlock); }

#include "host_path.h"

}  // namespace

namespace {
struct Family;  // below

// The model of one engine, as its family defines it in its engine_*.h: device buffers (DevPtr members, freed by the destructor), host
// tables and whatever the reference's model object counts per stream.  Made by Family::allocate, destroyed by free_all.
struct FamilyState {
  virtual ~FamilyState() = default;
};

template <class T>
void dfree(T*& p) {
  if (p) (void)hipFree(p), p = nullptr;
}

// A device buffer owned by a family's state struct: freed with the struct.  A chunked model (model_allocate) is not hipFree's to
// release: free_all nulls `p` through VmmRange::owner and releases the range BEFORE the state is destroyed.
template <class T>
struct DevPtr {
  T* p = nullptr;
  DevPtr() = default;
  DevPtr(DevPtr&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevPtr& operator=(DevPtr&& o) noexcept {
    std::swap(p, o.p);
    return *this;
  }
  DevPtr(const DevPtr&) = delete;
  DevPtr& operator=(const DevPtr&) = delete;
  ~DevPtr() { reset(); }
  void reset() { dfree(p); }
  operator T*() const { return p; }
};

#include "frame_history.h"

// The frame history ring of FrameDifference (2 slots) and WeightedMovingMean / Variance (3): the frame a stream receives at position
// `pos` lives in slot[pos % nring] + `off`, the stream's bytes into a slot (frame_history.h has the arithmetic).  Every engine has one
// (its classes' ring; the generic clip and host paths drive it), every group ONE for its fused classes.
struct FrameHistory {
  DevPtr<uint8_t> slot[3];
  int nring = 0;  // 0: the owner's classes keep no history
  enum Mode { kPrivate, kBorrowed, kClip } mode = kPrivate;  // kBorrowed: BGS_OPT_BORROW_FRAMES, the caller's previous d_frames are the history, no copies
  const uint8_t* lent[2] = {nullptr, nullptr};               // kBorrowed / kClip: frames t-1 and t-2

  // For the length of one call, whatever the owner's mode: Scope(h) - the call keeps private copies (the host entry points: their staging
  // buffer is reused every frame); Scope(h, h1, h2) - its history is these two frames (a clip call).  Restored on every return path.
  struct Scope {
    FrameHistory& h;
    const Mode mode;
    const uint8_t* const lent[2];
    explicit Scope(FrameHistory& h_) : h(h_), mode(h_.mode), lent{h_.lent[0], h_.lent[1]} { h.mode = kPrivate; }
    Scope(FrameHistory& h_, const uint8_t* h1, const uint8_t* h2) : Scope(h_) { h.mode = kClip, h.lent[0] = h1, h.lent[1] = h2; }
    ~Scope() { h.mode = mode, h.lent[0] = lent[0], h.lent[1] = lent[1]; }
    Scope(const Scope&) = delete;
  };

  void release() { slot[0].reset(), slot[1].reset(), slot[2].reset(); }
  // the question of both lock-step refusals: the caller's buffers hold one frame of ALL streams, a launch must cover them all at one age
  bool lockstep_only() const { return nring && mode == kBorrowed; }
  uint8_t* at(int i, size_t off) const { return i == kNoSlot ? nullptr : slot[i] + off; }
  // where the frame received at `pos` is kept; the k-th last frame before it of a stream that has seen t frames; the state planes
  // prev1 / prev2.  Null where there is no such slot (no ring, warm-up, another plane)
  uint8_t* keep_at(int64_t pos, size_t off) const { return at(nring ? history_cur(nring, pos) : kNoSlot, off); }
  const uint8_t* prev(int64_t pos, int64_t t, int k, size_t off) const { return at(history_prev(nring, pos, t, k), off); }
  const uint8_t* plane(int64_t pos, int64_t t, const char* name, size_t off) const { return at(history_plane(nring, pos, t, name), off); }
  // The history of one launch over `bytes` of frames at d_frames, received at `pos` by streams that have seen t: the frame is copied
  // into its slot unless it is there already (the host path uploads into it) or the history is lent; then the lent pair moves on.
  struct Frames { const uint8_t *cur, *h1, *h2; };
  hipError_t resolve(int64_t pos, int64_t t, size_t off, size_t bytes, const uint8_t* d_frames, hipStream_t s, Frames* f) {
    *f = {d_frames, nring ? lent[0] : nullptr, nring ? lent[1] : nullptr};
    if (!nring) return hipSuccess;
    if (mode != kPrivate) return lent[1] = lent[0], lent[0] = d_frames, hipSuccess;
    uint8_t* own = keep_at(pos, off);
    *f = {own, prev(pos, t, 1, off), prev(pos, t, 2, off)};
    return own == d_frames ? hipSuccess : hipMemcpyAsync(own, d_frames, bytes, hipMemcpyDeviceToDevice, s);
  }
};

// Kernel timing: one event pair per timed launch (Timed, below).  Bounded: a caller that leaves this measurement aid on must not grow the list forever.
struct LaunchTimer {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  bool full() const { return events.size() >= 16384; }
  void enable(bool v) {
    for (auto& ev : events) (void)hipEventDestroy(ev.first), (void)hipEventDestroy(ev.second);
    events.clear(), on = v;
  }
  ~LaunchTimer() { enable(false); }
  // ms of the first `cap` pairs: their number, their sum, each one into `each` when given.  wait: every pair's end event is waited for
  // and a HIP error ends the walk (the engine's calls); else the device is drained and a pair that cannot be read counts as 0 ms
  hipError_t read(bool wait, int64_t cap, float* each, int64_t* n, double* total) const {
    for (*n = 0, *total = 0; *n < cap && *n < (int64_t)events.size(); ++*n) {
      const auto& ev = events[(size_t)*n];
      float ms = 0;
      hipError_t er = wait ? hipEventSynchronize(ev.second) : hipSuccess;
      if (er == hipSuccess) er = hipEventElapsedTime(&ms, ev.first, ev.second);
      if (wait && er != hipSuccess) return er;
      if (each) each[*n] = ms;
      *total += ms;
    }
    return hipSuccess;
  }
};
}

// One virtual address range backed by separately created physical chunks (hipMemAddressReserve + hipMemCreate x n + hipMemMap): how
// the big models are placed (model_allocate) and what bgs_calibrate_copy measures beside a plain hipMalloc.
struct VmmRange {
  std::vector<hipMemGenericAllocationHandle_t> handles;
  void* base = nullptr;
  void** owner = nullptr;  // the raw pointer inside the DevPtr that model_allocate filled with `base` (free_all nulls it: the range is not hipFree's to release)
  size_t bytes = 0, chunk = 0, mapped = 0;  // mapped: chunks actually mapped (a failure half-way leaves fewer than handles)
};

// What is here is what the generic code below uses itself.  A family's model - buffers, tables, per-stream counters - is the state
// struct of its engine_*.h behind `model`; what stays is
//  - geometry, the per-stream bookkeeping every family shares (seen, rpos, last_flags), the host path (HostPath), timing (LaunchTimer), ingest, cc scratch, vmm;
//  - `hist`, the frame history ring (FrameHistory, above): process_clip_run and the host entry points say for the length of a call where its
//    history comes from (FrameHistory::Scope) and upload into its slots, so it is a service of the generic code that the history classes
//    use (ring_run asks it for the frames of a launch), not their private state; a group holds the same struct;
//  - `counter`: the families that have a learning phase counted in frames share it with that one meaning, and bgs_reset_stream clears it;
//  - p and the class parameter blocks (one member per ParamBlock constant of an engine_*.h, which says who owns it and whether it
//    is live or frozen once the geometry is set): all may be set before the geometry is known, i.e. before there is a state;
//  - the knobs, which bgs_create (environment) and bgs_set_option set before allocation.
struct bgs_engine {
  bgs_algo algo;
  const Family* fam = nullptr;  // the class's entry points (family_of)
  std::unique_ptr<FamilyState> model;  // the class's state (null until the geometry is set, and for the frame history classes)
  bgs_params p;
  bgs_fuzzy_params fz{};       // kFuzzyBlock
  bgs_t2f_params t2f{};        // kT2fBlock
  bgs_eigen_params eig{};      // kEigenBlock
  bgs_imbs_params imbs{};      // kImbsBlock
  bgs_multilayer_params ml{};  // kMultilayerBlock
  int device = 0;
  int n_cu = 256;  // compute units of `device` (allocate): the persistent kernels size their grids by it
  int S = 1;
  int rows = 0, cols = 0, ch = 0;
  size_t n = 0;  // pixels per stream; 0 until the geometry is known
  std::vector<int64_t> seen, counter;
  std::vector<int64_t> rpos;         // frame history ring: the position of a stream's NEXT frame (hist); survives bgs_reset_stream, so that streams fed in the same calls keep sharing launches
  std::vector<uint32_t> last_flags;  // out_flags of each stream's last frame (bgs_stream_flags)
  FrameHistory hist;                 // FD: 2 slots, WMM / WMV: 3, every other class: none

  struct Knobs {
    int xcd_swizzle = 1;             // XCD-aware block order (kernel_mog2.h): 0 off, 1 model kernels (MOG2, MOG1, dp), 2 also the byte-stream kernels
    int mog2_sparse = 3;             // data-dependent traffic (kernel_mog2.h): 0 dense (everything loaded and written), 1 only what changed is written, 2 / 4 a lane also loads only the modes its pixel has, 3 = choose 1 or 4 from the scene
    int mog2_complete = 1;           // sector-complete stores (kernel_mog2.h); BGS_MOG2_COMPLETE=0 for A/B runs
    bool clip_fuse = true;           // clip calls of the families with a clip_fused entry keep the model in registers across frames (option 7; results identical either way)
    int lb_px = 1;                   // pixels per lane of the two Gaussian kernels (BGS_LB_PX=2: the double2 form, A/B; identical results)
    int vu_sparse = 1;               // BGS_VU_SPARSE: 0 dense, 1 live-bin with whole-line stores, 2 live-bin with masked stores (identical results)
    bool kde_count_trips = false;    // diagnostics: count density-loop trips (BGS_KDE_TRIPS=1)
    int model_chunk_mb = 256;        // big models are built from physical chunks of this size (model_allocate); 0: one plain hipMalloc
    size_t model_chunk_min_bytes = (size_t)768 << 20;  // models below this take one plain hipMalloc (BGS_MODEL_CHUNK_MIN_MB: test knob)
    bool poison = false;             // BGS_DEBUG_POISON: every fresh device buffer is filled with 0xA5 (see dmalloc)
    int host_register = 0;           // BGS_OPT_HOST_REGISTER: roles that may be page-locked in place (bit 0 input, 1 mask, 2 background); 0 = always stage
  } knob;
  // a model built from fixed-size physical chunks with the virtual memory API (model_allocate)
  VmmRange vmm;

  HostPath host;                          // everything of the calls that take frames in host memory (host_path.h)
  hipStream_t stream() const { return host.sync.hs; }  // the engine's own stream is its synchronous lane's; made by allocate(), where families enqueue their table uploads
  bool ingest_on = false;             // bgs_set_ingest: bgs_process takes raw frames
  bgs_ingest ingest{};
  int raw_rows = 0, raw_cols = 0;     // geometry of the raw frames (fixed by the first one)
  uint8_t* pack_fg = nullptr;         // frames of rows*cols % 64 != 0 pixels: the byte masks a packed-only caller's bit masks are made from
  size_t pack_fg_bytes = 0;
  int last_fg_stream = -1;            // bgs_last_mask_blobs: whose mask host.sync.fg.d holds (-1: none valid)
  void* cc_work = nullptr;            // its device scratch: workspace | boxes | moments | count
  int cc_cap = 0;                     // boxes the scratch has room for

  LaunchTimer timer;                  // dominant-kernel timing
  const char* kernel_name = "";
};

namespace {

// What a class of background model plugs into the engine: one constant of this per family at the end of its engine_*.h, found by
// family_of().  `first`, `count`: a run of streams that share every kernel argument (launch_key); d_* point at the run's first
// stream.  Entries marked nullable may stay null.  A family whose parameters are not bgs_params puts a ParamBlock constant (below)
// beside it.
struct Family {
  int (*check)(bgs_algo, const bgs_params&);                      // nullable; needs no device (bgs_create, bgs_set_params)
  int (*check_geometry)(bgs_algo, int rows, int cols, int ch);    // nullable; refusals made before the device is opened
  int (*allocate)(bgs_engine*);                                   // rows / cols / ch / n are set, e->stream() exists; makes e->model (make_state) and fills it; after a failure free_all destroys what there is of it
  uint64_t (*key)(const bgs_engine*, int stream);                 // streams whose next frame has the same key share a launch
  // one frame: launches on s, advances the family's own per-stream counters, *flags = BGS_FG_VALID / BGS_BG_VALID of the run
  int (*run)(bgs_engine*, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags);
  int64_t (*get_state)(bgs_engine*, int stream, const char* plane, void* dst, size_t cap);
  void (*reset_stream)(bgs_engine*, int stream);                  // nullable; per-stream counters of the state beyond seen / counter / last_flags (called only when there is a state)
  void (*keep_frozen)(bgs_params& p, const bgs_params& old);      // nullable; what bgs_set_params restores once the geometry is set
  int (*apply_params)(bgs_engine*);                               // nullable; device tables that follow live parameters (bgs_set_params)
  bool (*needs_byte_mask)(const bgs_engine*);                     // nullable (no); the packed mask is made from the finished byte mask
  // nullable; `fuse` = 2, 4 or 8 consecutive frames of a clip in one launch that keeps the model in registers; slab: pixels from one
  // frame of the clip to the next.  Taken when clip_fusable (nullable: always) agrees.
  int (*clip_fused)(bgs_engine*, int first, int count, int fuse, size_t slab, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* flags);
  bool (*clip_fusable)(const bgs_engine*);
  int bg_channels;        // channels of the background image the class hands out: 0 = as the frames, 1 = gray
  bool per_stream_flags;  // run writes e->last_flags[first..first+count) itself and returns their AND (streams of one launch differ)
};

const Family* family_of(bgs_algo algo);  // below

// The parameters of a class that do not fit in bgs_params are a block of its own: an ABI struct P that begins with struct_size, held
// by the engine as `member`.  Its family describes it once, in one constant of this next to its Family; the four entry points of the
// block (bgs_<x>_default_params, bgs_set_<x>_params, bgs_get_<x>_params, bgs_<x>_check) are block_default / block_set / block_get /
// block_check on that constant, and for_each_block lists it for bgs_create and bgs_group_create.
template <class P>
struct ParamBlock {
  P bgs_engine::*member;
  const Family* fam;        // the block belongs to the classes of this family
  const char* struct_name;  // of P, for the struct_size refusal
  const char* class_name;   // of the owning classes, for the wrong-class refusal
  void (*defaults)(P*);
  int (*check)(bgs_algo, const P&);  // needs no device; the geometry refusals are fam->check_geometry
  bool live;  // a set after the geometry: true = acts from the next frame on, false = vetted, then ignored (the model keeps what it was built with)
};

// what the caller handed in, or the block's defaults (kept in d) for NULL; null after refusing a struct of another size
template <class P>
const P* block_arg(const ParamBlock<P>& b, const P* p, P& d) {
  if (!p) return b.defaults(&d), &d;
  if (p->struct_size != sizeof(P)) return fail(BGS_ERR_INVALID, "%s.struct_size %u != %zu (ABI mismatch)", b.struct_name, p->struct_size, sizeof(P)), nullptr;
  return p;
}

// the refusals that need no engine, in the order the ABI promises: wrong class, struct_size, the family's check
template <class P>
int block_vet(const ParamBlock<P>& b, const char* fn, bgs_algo algo, const P* p) {
  if (family_of(algo) != b.fam) return fail(BGS_ERR_INVALID, "%s: algorithm %d is not %s", fn, (int)algo, b.class_name);
  P d;
  p = block_arg(b, p, d);
  return p ? b.check(algo, *p) : BGS_ERR_INVALID;
}

template <class P>
int block_default(const ParamBlock<P>& b, P* p) {
  if (!p) return fail(BGS_ERR_INVALID, "params is NULL");
  b.defaults(p);
  return BGS_OK;
}

template <class P>
int block_set(const ParamBlock<P>& b, const char* fn, bgs_engine* e, const P* p) {
  if (!e || !p) return fail(BGS_ERR_INVALID, "NULL argument");
  int rc = block_vet(b, fn, e->algo, p);
  if (rc) return rc;
  if (b.live || !e->n) e->*b.member = *p;
  return BGS_OK;
}

template <class P>
int block_get(const ParamBlock<P>& b, const char* fn, const bgs_engine* e, P* p) {
  if (!e || !p) return fail(BGS_ERR_INVALID, "NULL argument");
  if (e->fam != b.fam) return fail(BGS_ERR_INVALID, "%s: algorithm %d is not %s", fn, (int)e->algo, b.class_name);
  *p = e->*b.member;
  return BGS_OK;
}

// p NULL: the defaults; rows <= 0: the parameters alone
template <class P>
int block_check(const ParamBlock<P>& b, const char* fn, bgs_algo algo, const P* p, int rows, int cols, int ch) {
  int rc = block_vet(b, fn, algo, p);
  if (rc || rows <= 0 || !b.fam->check_geometry) return rc;
  return b.fam->check_geometry(algo, rows, cols, ch);
}

void vmm_free(VmmRange& v);  // below

int bg_channels(const bgs_engine* e) { return e->fam->bg_channels ? e->fam->bg_channels : e->ch; }

// OR of the flags of the last frame of streams [first, first+count): did any of them produce a mask
uint32_t any_flags(const bgs_engine* e, int first, int count) {
  uint32_t any = 0;
  for (int i = first; i < first + count; ++i) any |= e->last_flags[i];
  return any;
}

bool always(const bgs_engine*) { return true; }  // needs_byte_mask of the classes whose mask is finished by a stencil pass

// the state of e's family: made by its allocate, typed again by the one-line accessor of its engine_*.h
template <class St>
St& make_state(bgs_engine* e) {
  St* st = new St();
  e->model.reset(st);
  return *st;
}
template <class St>
St& state_of(const bgs_engine* e) {
  return static_cast<St&>(*e->model);
}

// bgs_get_state.  fetch: device memory into scratch of the library's own; too_small: the refusal of a caller's buffer, made before
// anything is read back; copy_plane / copy_host: `nb` bytes of device memory / of a value the host already holds are plane `plane`
int fetch(void* dst, const void* src, size_t nb) { return d2h_staged(dst, src, nb) == BGS_OK ? BGS_OK : fail(BGS_ERR_HIP, "hipMemcpy failed"); }
int64_t too_small(const char* plane) { return fail(BGS_ERR_STATE, "buffer too small for plane %s", plane); }
int64_t copy_plane(const char* plane, void* dst, size_t cap, const void* src, size_t nb) {
  if (cap < nb) return too_small(plane);
  return fetch(dst, src, nb) ? BGS_ERR_HIP : (int64_t)nb;
}
int64_t copy_host(const char* plane, void* dst, size_t cap, const void* src, size_t nb) {
  if (cap < nb) return too_small(plane);
  std::memcpy(dst, src, nb);
  return (int64_t)nb;
}
int64_t unknown_plane(const bgs_engine* e, const char* plane) { return fail(BGS_ERR_STATE, "unknown state plane '%s' for algorithm %d", plane, (int)e->algo); }

// Every model / history / staging buffer of an engine comes from here.  Nothing may rely on what a fresh allocation holds:
// each model is initialised at a stream's first frame ON THE LAUNCH STREAM (mog2_clear, mog1_clear_kernel, gmg_clear_kernel,
// dp_gmm_clear_kernel, ss_init_streams, ...).  BGS_DEBUG_POISON=1 makes a violation deterministic instead of timing- and
// allocator-dependent: the buffer is filled with 0xA5 (a NaN-free but wildly wrong float, a mode count of 165) before first use.
int dmalloc(bgs_engine* e, void** p, size_t bytes) {
  HIP_TRY(hipMalloc(p, bytes));
  if (e->knob.poison) HIP_TRY(hipMemsetAsync(*p, 0xA5, bytes, e->stream()));  // allocate() drains e->stream() before it returns
  return BGS_OK;
}
template <class T>
void** raw_of(T*& p) { return (void**)&p; }
template <class T>
void** raw_of(DevPtr<T>& d) { return (void**)&d.p; }
#define DMALLOC(ptr, bytes)                               \
  do {                                                    \
    int rc__ = dmalloc(e, raw_of(ptr), (bytes));          \
    if (rc__) return rc__;                                \
  } while (0)

// the launches between its construction and its destruction on s, as one pair of the timer (an engine's: with the kernel's name)
struct Timed {
  LaunchTimer& tm;
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  Timed(LaunchTimer& tm_, hipStream_t s_, bool enable = true) : tm(tm_), s(s_) {
    if (enable && tm.on && !tm.full() && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, s);
  }
  Timed(bgs_engine* e, hipStream_t s_, const char* name, bool enable = true) : Timed(e->timer, s_, enable) {
    if (enable) e->kernel_name = name;
  }
  ~Timed() {
    if (a && b) {
      (void)hipEventRecord(b, s);
      tm.events.emplace_back(a, b);
    }
  }
};

// Model allocation for the big, long-lived models (MOG2, MOG1, dp): ONE virtual range backed by separately created physical chunks.
// Measured on MI355X in rounds 1-3 (profiles/r02_placement_probe.txt, profiles/r03_placement.txt): the same kernel on
// the same layout streamed a multi-GB model at one of 2-3 speeds, 8-10 % apart, depending on which physical VRAM one big hipMalloc
// handed out - a physically contiguous run above ~1 GiB, which a LATER large hipMalloc of a long-lived process tends to get, was the
// slow one.  Rounds 1-2 looked for a fast placement by trial (up to 20 candidates of the whole model allocated and timed); round 3
// found that chunks of at most 1 GiB (hipMemCreate / hipMemMap) never land there: 15 of 15 fresh processes at 1.103-1.110 ms per
// launch for chunk sizes 2 MiB .. 1 GiB, 3 of 3 slow with 4 GiB chunks, plain hipMalloc 1.11 1.11 1.12 1.19 1.21 1.21.
// Round 4 checked the claim from the other side (bench.py `calibration`, the round-3 verdict's question): a float4 copy through a chunked
// range is NOT faster than through a fresh plain allocation (6.14-6.21 against 6.19-6.27 TB/s on every box) - the construction does
// not buy bandwidth, it avoids the bad placement - and it does not explain the 6-9 % between BOXES of the pool, which show the same
// copy rate.  So: chunks of 256 MiB (BGS_MODEL_CHUNK_MB; 0 = one plain hipMalloc), no probe, no transient memory.
int vmm_allocate(VmmRange& v, int device, void** out, size_t bytes, size_t chunk) {
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  size_t gran = 0;
  HIP_TRY(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
  if (!gran) gran = 2u << 20;
  chunk = (chunk + gran - 1) / gran * gran;
  const size_t total = (bytes + chunk - 1) / chunk * chunk;
  void* base = nullptr;
  HIP_TRY(hipMemAddressReserve(&base, total, 0, nullptr, 0));
  v.base = base, v.bytes = total, v.chunk = chunk, v.mapped = 0;
  for (size_t off = 0; off < total; off += chunk) {
    hipMemGenericAllocationHandle_t h;
    HIP_TRY(hipMemCreate(&h, chunk, &prop, 0));
    v.handles.push_back(h);
    HIP_TRY(hipMemMap((char*)base + off, chunk, 0, h, 0));
    v.mapped++;  // vmm_free unmaps exactly the (address, size) pairs that were mapped, also after a failure half-way
  }
  hipMemAccessDesc acc = {};
  acc.location = prop.location;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  HIP_TRY(hipMemSetAccess(base, total, &acc, 1));
  *out = base;
  return BGS_OK;
}
void vmm_free(VmmRange& v) {
  if (!v.base) return;
  // HIP's virtual memory API is Beta: release in the portable order - every chunk unmapped with the (address, size) it was mapped
  // with, then every handle released, then the range freed - and say so when a step fails (a silent failure here leaks gigabytes)
  auto warn = [](const char* what, hipError_t er) {
    if (er != hipSuccess) {
      fprintf(stderr, "[bgs] %s failed while releasing a chunked range: %s\n", what, hipGetErrorString(er));
      (void)hipGetLastError();
    }
  };
  for (size_t i = 0; i < v.mapped; ++i) warn("hipMemUnmap", hipMemUnmap((char*)v.base + i * v.chunk, v.chunk));
  for (auto& h : v.handles) warn("hipMemRelease", hipMemRelease(h));
  warn("hipMemAddressFree", hipMemAddressFree(v.base, v.bytes));
  v.handles.clear(), v.base = nullptr, v.owner = nullptr, v.bytes = 0, v.mapped = 0;
}

// A model of `bytes`: chunked (see above) from 768 MB up - smaller ones sit in the 256 MiB Infinity Cache for a good part and are
// not HBM-bound - else, or when the virtual memory API refuses, one hipMalloc.  An engine has at most one such model.
int model_allocate(bgs_engine* e, void** out, size_t bytes) {
  if (e->knob.model_chunk_mb > 0 && bytes >= e->knob.model_chunk_min_bytes && !e->vmm.base) {
    if (vmm_allocate(e->vmm, e->device, out, bytes, (size_t)e->knob.model_chunk_mb << 20) == BGS_OK) {
      e->vmm.owner = out;
      if (e->knob.poison) HIP_TRY(hipMemsetAsync(*out, 0xA5, e->vmm.bytes, e->stream()));
      return BGS_OK;
    }
    (void)hipGetLastError();
    vmm_free(e->vmm);  // whatever part of it came to be
    *out = nullptr;
  }
  return dmalloc(e, out, bytes);
}
template <class T>
int model_allocate(bgs_engine* e, DevPtr<T>& out, size_t bytes) { return model_allocate(e, raw_of(out), bytes); }

// cv::getGaussianKernel(n, sigma, CV_32F) for sigma > 0 (imgproc/src/smooth.cpp): the taps in float, their sum in double
void gaussian_kernel_f32(int n, double sigma, float* cf) {
  const double scale2X = -0.5 / (sigma * sigma);
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    cf[i] = (float)std::exp(scale2X * x * x);
    sum += cf[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < n; ++i) cf[i] = (float)(cf[i] * sum);
}

// The families.  Order matters where one borrows from another: engine_asbl.h uses engine_pointwise.h's launch macro, engine_mog2.h
// uses engine_mog1.h's launch key.
#include "engine_pointwise.h"
#include "engine_asbl.h"
#include "engine_gmg.h"
#include "engine_mog1.h"
#include "engine_mog2.h"
#include "engine_subsense.h"
#include "engine_dp.h"
#include "engine_kde.h"
#include "engine_dp2.h"
#include "engine_lb.h"
#include "engine_vumeter.h"
#include "engine_fuzzy.h"
#include "engine_t2f.h"
#include "engine_eigen.h"
#include "engine_imbs.h"
#include "engine_multilayer.h"
#include "engine_multicue.h"

// an id that BGS_ALGO_KNOWN accepts but no engine class stands behind (BGS_LBSP_DESC is a stand-alone entry point): refused when the geometry is set
constexpr Family kUnbuilt = [] {
  Family f{};
  f.allocate = [](bgs_engine* e) -> int { return fail(BGS_ERR_UNSUPPORTED, "algorithm %d is not implemented in this build", (int)e->algo); };
  return f;
}();

// THE table: which family stands behind an id.  No default: an enumerator nobody wired in is -Wall's switch warning.
const Family* family_of(bgs_algo algo) {
  switch (algo) {
    case BGS_FRAME_DIFF:
    case BGS_WMM:
    case BGS_WMV: return &kFrameHistory;
    case BGS_STATIC_FRAME_DIFF: return &kStaticFrameDiff;
    case BGS_ABL: return &kAbl;
    case BGS_ASBL: return &kAsbl;
    case BGS_SIGMA_DELTA: return &kSigmaDelta;
    case BGS_GMG: return &kGmg;
    case BGS_MOG1: return &kMog1;
    case BGS_MOG2: return &kMog2;
    case BGS_SUBSENSE: return &kSubsense;
    case BGS_LOBSTER: return &kLobster;
    case BGS_DP_ZIVKOVIC_AGMM:
    case BGS_DP_GRIMSON_GMM:
    case BGS_DP_WREN_GA:
    case BGS_DP_MEAN:
    case BGS_DP_ADAPTIVE_MEDIAN: return &kDp;
    case BGS_KDE: return &kKde;
    case BGS_DP_PRATI_MEDIOD: return &kDpPratiMediod;
    case BGS_DP_TEXTURE: return &kDpTexture;
    case BGS_LB_SIMPLE_GAUSSIAN:
    case BGS_LB_FUZZY_GAUSSIAN:
    case BGS_LB_MOG:
    case BGS_LB_ADAPTIVE_SOM:
    case BGS_LB_FUZZY_ADAPTIVE_SOM: return &kLb;
    case BGS_VUMETER: return &kVuMeter;
    case BGS_FUZZY_SUGENO:
    case BGS_FUZZY_CHOQUET: return &kFuzzy;
    case BGS_T2FGMM_UM:
    case BGS_T2FGMM_UV: return &kT2f;
    case BGS_DP_EIGENBACKGROUND: return &kEigen;
    case BGS_IMBS: return &kImbs;
    case BGS_MULTILAYER: return &kMultilayer;
    case BGS_LBSP_DESC:
    case BGS_ALGO_END:
    case BGS_ALGO_LIMIT:
    case BGS_ALGO_LAST: break;
  }
  return &kUnbuilt;
}

// Every class parameter block: bgs_create sets each to its defaults, bgs_group_create refuses the classes that own one.
template <class F>
void for_each_block(F f) {
  f(kFuzzyBlock), f(kT2fBlock), f(kEigenBlock), f(kImbsBlock), f(kMultilayerBlock);
}

void free_all(bgs_engine* e) {
  if (e->vmm.base) {  // a model built by model_allocate from physical chunks is not hipFree's to release: its DevPtr is emptied before the state goes
    if (e->vmm.owner) *e->vmm.owner = nullptr;
    vmm_free(e->vmm);
  }
  e->model.reset();
  e->hist.release();
  dfree(e->cc_work), e->cc_cap = 0;
  dfree(e->pack_fg), e->pack_fg_bytes = 0;
  e->last_fg_stream = -1;
  e->host.release();
}

int check_params(bgs_algo algo, const bgs_params& p) {
  const Family* f = family_of(algo);
  return f->check ? f->check(algo, p) : BGS_OK;
}

// the refusals of a geometry, made before the device is opened: those of every class, then the family's (an engine's own; a group's fused SigmaDelta)
int check_geometry(const Family* fam, bgs_algo algo, int rows, int cols, int ch) {
  if (rows <= 0 || cols <= 0) return fail(BGS_ERR_INVALID, "bad geometry %dx%d", rows, cols);
  if (ch != 1 && ch != 3) return fail(BGS_ERR_UNSUPPORTED, "channels must be 1 or 3, got %d", ch);
  return fam && fam->check_geometry ? fam->check_geometry(algo, rows, cols, ch) : BGS_OK;
}

int allocate(bgs_engine* e, int rows, int cols, int ch) {
  int rc = check_geometry(e->fam, e->algo, rows, cols, ch);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));
  e->rows = rows, e->cols = cols, e->ch = ch, e->n = (size_t)rows * cols;
  HIP_TRY(e->host.sync.open());  // e->stream()
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, e->device) == hipSuccess && prop.multiProcessorCount > 0) e->n_cu = prop.multiProcessorCount;
  rc = e->fam->allocate(e);
  if (rc) return rc;
  // Whatever allocation enqueued on e->stream() (statistics counters, poison fills) is complete before the caller's first
  // launch - which may come on ANOTHER stream (device path) that nothing else orders against this one.
  HIP_TRY(hipStreamSynchronize(e->stream()));
  return BGS_OK;
}

bool host_pin(bgs_engine* e, int stream, int role, const void* ptr, size_t bytes, hipStream_t s) { return e->host.pinned(e->knob.host_register, stream, role, ptr, bytes, s); }

// The staging of a camera's lane (the synchronous one or a bgs_submit lane), sized by the geometry; made by the first call that needs it
int lane_make(bgs_engine* e, Lane& ln, const char* fn, int stream) {
  if (ln.done) return BGS_OK;
  const size_t bytes[3] = {e->n * e->ch, e->n, e->n * bg_channels(e)};
  const hipError_t er = ln.make(bytes[0], bytes[1], bytes[2]);
  if (er != hipSuccess) return fail(BGS_ERR_HIP, "%s: setting up the lane of stream %d failed: %s", fn, stream, hipGetErrorString(er));
  const Staging* st[3] = {&ln.in, &ln.fg, &ln.bg};
  for (int i = 0; i < 3 && e->knob.poison; ++i) HIP_TRY(hipMemsetAsync(st[i]->d, 0xA5, bytes[i], ln.hs));  // see dmalloc
  return BGS_OK;
}

// What one launch can cover: streams whose next frame needs the same kernel arguments share a RUN.  Cameras come and go
// independently (the reference creates and deletes one IBGS object per stream whenever it likes: FrameProcessor.cpp:35-155,
// :342-482; ustc_src/ustc_bgs.cpp:75-77), so the streams of a batch may have seen different numbers of frames; what a launch
// depends on is far less than the age - e.g. for MOG2 only "first frame?" and the learning rate, which with the wrapper's fixed
// alpha is the same from a stream's second frame on.  Streams in lock-step (the benchmark, any batch fed by whole-batch calls) are
// one run = one launch, exactly as before.
uint64_t launch_key(const bgs_engine* e, int i) { return e->fam->key(e, i); }

// their packed mask is always made from the finished byte mask (median after the pixel loop)
bool needs_byte_mask(const bgs_engine* e) { return e->fam->needs_byte_mask && e->fam->needs_byte_mask(e); }

int process_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s, uint32_t* out_flags);

// engine-owned byte masks for packed-only callers of frames whose pixel count is not a multiple of 64 (see process_range); grown on
// demand, ordered on the call's stream like every other engine buffer
int pack_scratch(bgs_engine* e, size_t bytes, hipStream_t s) {
  if (e->pack_fg_bytes >= bytes) return BGS_OK;
  if (e->pack_fg) {
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipFree(e->pack_fg), e->pack_fg = nullptr, e->pack_fg_bytes = 0;
  }
  HIP_TRY(hipMalloc((void**)&e->pack_fg, bytes));
  e->pack_fg_bytes = bytes;
  return BGS_OK;
}
void pack_ragged(bgs_engine* e, const uint8_t* fg, uint64_t* bits, size_t images, hipStream_t s) {
  const size_t W = (e->n + 63) / 64;
  hipLaunchKernelGGL(bgs::mask_pack_ragged_kernel, dim3(blocks_for(images * W * bgs::kWave)), dim3(bgs::kBlock), 0, s, fg, bits, e->n, W, images);
}

// One frame for streams [first, first+count), device pointers, asynchronous on s: one launch per run of streams (see launch_key).
int process_range(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s,
                  uint32_t* out_flags) {
  if (out_flags) *out_flags = 0;
  if (!e->n) return fail(BGS_ERR_INVALID, "geometry not set: call bgs_set_geometry or bgs_process first");
  if (first < 0 || count <= 0 || first + count > e->S) return fail(BGS_ERR_INVALID, "stream range [%d,%d) outside 0..%d", first, first + count, e->S);
  if (!d_frames) return fail(BGS_ERR_INVALID, "d_frames is NULL");
  // Packed masks: stream k of the call owns words [k W, (k + 1) W), W = ceil(rows*cols / 64).  When rows*cols is a multiple of 64
  // (1080p, 4K, 720p, VGA, the reference's 320x176 video ...) the kernels write the words themselves from wave ballots; otherwise a
  // wave's 64 pixels straddle two words (and two streams), so the kernels write byte masks - the caller's d_fg, or the engine's own
  // buffer when it passed none - and mask_pack_ragged_kernel makes the words from them, tail bits zero.
  const size_t W = (e->n + 63) / 64;
  const bool ragged = d_bits && (e->n % 64) != 0;
  if (d_bits && !d_fg && (ragged || needs_byte_mask(e))) {
    int rc = pack_scratch(e, (size_t)count * e->n, s);
    if (rc) return rc;
    d_fg = e->pack_fg;
  }
  uint32_t all = ~0u;
  const size_t C = (size_t)e->ch, bgC = (size_t)bg_channels(e);
  for (int a = first; a < first + count;) {
    int b = a + 1;
    const uint64_t key = launch_key(e, a);
    while (b < first + count && launch_key(e, b) == key) ++b;
    if (e->hist.lockstep_only() && (a != first || b != first + count))
      return fail(BGS_ERR_INVALID, "borrowed frame history needs streams in lock-step (streams %d and %d are not)", a, b);
    const size_t o = (size_t)(a - first) * e->n;
    uint32_t fl = 0;
    int rc = process_run(e, a, b - a, d_frames + o * C, d_fg ? d_fg + o : nullptr, d_bg ? d_bg + o * bgC : nullptr, (d_bits && !ragged) ? d_bits + (size_t)(a - first) * W : nullptr, s, &fl);
    if (rc) return rc;
    if (ragged && (any_flags(e, a, b - a) & BGS_FG_VALID)) pack_ragged(e, d_fg + o, d_bits + (size_t)(a - first) * W, (size_t)(b - a), s);
    all &= fl;
    a = b;
  }
  if (out_flags) *out_flags = all;  // what holds for every stream of the range; per stream: bgs_stream_flags
  return BGS_OK;
}

// One frame for a run of streams that share every kernel argument.
int process_run(bgs_engine* e, int first, int count, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s,
                uint32_t* out_flags) {
  if (out_flags) *out_flags = 0;
  HIP_TRY(hipSetDevice(e->device));
  if (d_bits && (e->n * count) % 64) return fail(BGS_ERR_INVALID, "internal: a ragged packed mask reached process_run");  // process_range packs those itself
  uint32_t flags = 0;
  int rc = e->fam->run(e, first, count, d_frames, d_fg, d_bg, d_bits, s, &flags);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  for (int i = first; i < first + count; ++i) {
    e->seen[i]++, e->rpos[i]++;
    if (!e->fam->per_stream_flags) e->last_flags[i] = flags;
  }
  if (out_flags) *out_flags = flags;
  return BGS_OK;
}


// bgs_process_clip_device: `nframes` consecutive frames of streams [first, first+count).  Every algorithm: frame by frame
// through process_range (the same launches as nframes range calls).  Families with a clip_fused entry (MOG2, MOG1, the dp GMMs,
// T2FGMM_UM / T2FGMM_UV, the five lb/ classes): runs of 8 / 4 / 2 frames go through ONE launch that keeps the model in registers;
// what is left over takes the single-frame kernel.
int process_clip_run(bgs_engine* e, int first, int count, int slab_count, int nframes, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits,
                     hipStream_t s, uint32_t* out_flags);

// The streams of a clip call may have different ages too: one pass per run of streams with the same age and launch arguments
// (launch_key); the frames of a run sit inside the caller's [nframes][count] slab, so a run keeps the slab's strides.
int process_clip(bgs_engine* e, int first, int count, int nframes, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits, hipStream_t s,
                 uint32_t* out_flags) {
  if (nframes < 1) return fail(BGS_ERR_INVALID, "nframes must be >= 1");
  if (!e->n) return fail(BGS_ERR_INVALID, "geometry not set: call bgs_set_geometry or bgs_process first");
  if (first < 0 || count <= 0 || first + count > e->S) return fail(BGS_ERR_INVALID, "stream range [%d,%d) outside 0..%d", first, first + count, e->S);
  if (!d_frames) return fail(BGS_ERR_INVALID, "d_frames is NULL");
  const size_t W = (e->n + 63) / 64;
  const bool ragged = d_bits && (e->n % 64) != 0;  // as in process_range: byte masks first, then mask_pack_ragged_kernel
  if (d_bits && !d_fg && (ragged || needs_byte_mask(e))) {
    int rc = pack_scratch(e, (size_t)nframes * count * e->n, s);
    if (rc) return rc;
    d_fg = e->pack_fg;
  }
  const size_t C = (size_t)e->ch, bgC = (size_t)bg_channels(e);
  std::vector<uint32_t> fl((size_t)nframes), all((size_t)nframes, ~0u);
  for (int a = first; a < first + count;) {
    int b = a + 1;
    while (b < first + count && e->seen[b] == e->seen[a] && launch_key(e, b) == launch_key(e, a)) ++b;
    const size_t o = (size_t)(a - first) * e->n;
    int rc = process_clip_run(e, a, b - a, count, nframes, d_frames + o * C, d_fg ? d_fg + o : nullptr, d_bg ? d_bg + o * bgC : nullptr, (d_bits && !ragged) ? d_bits + (size_t)(a - first) * W : nullptr, s, fl.data());
    if (rc) return rc;
    if (ragged)  // per frame only the AND over the run is known here (last_flags holds the clip's last frame): as before, a run that mixes learning and detecting streams of a per_stream_flags family gets no words
      for (int t = 0; t < nframes; ++t)
        if (fl[t] & BGS_FG_VALID) pack_ragged(e, d_fg + (size_t)t * count * e->n + o, d_bits + ((size_t)t * count + (size_t)(a - first)) * W, (size_t)(b - a), s);
    for (int t = 0; t < nframes; ++t) all[t] &= fl[t];
    a = b;
  }
  if (out_flags)
    for (int t = 0; t < nframes; ++t) out_flags[t] = all[t];
  return BGS_OK;
}

// `fuse` frames of a clip as ONE launch of the family (Family::clip_fused), which needs the streams of the run in lock-step
int clip_fused_run(bgs_engine* e, int first, int count, int fuse, size_t slab, const uint8_t* fr, uint8_t* fg, uint8_t* bg, uint64_t* bits, hipStream_t s, uint32_t* out_flags) {
  const int64_t seen = e->seen[first];
  for (int i = first; i < first + count; ++i)
    if (e->seen[i] != seen) return fail(BGS_ERR_INVALID, "streams %d and %d are not in lock-step (%lld vs %lld frames)", first, i, (long long)seen, (long long)e->seen[i]);
  HIP_TRY(hipSetDevice(e->device));
  uint32_t fl = 0;
  int rc = e->fam->clip_fused(e, first, count, fuse, slab, fr, fg, bg, bits, s, &fl);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  for (int i = first; i < first + count; ++i) e->seen[i] += fuse, e->rpos[i] += fuse, e->last_flags[i] = fl;
  for (int j = 0; j < fuse && out_flags; ++j) out_flags[j] = fl;
  return BGS_OK;
}

// `count` streams of one age starting at `first`, inside a slab of `slab_count` streams per frame
int process_clip_run(bgs_engine* e, int first, int count, int slab_count, int nframes, const uint8_t* d_frames, uint8_t* d_fg, uint8_t* d_bg, uint64_t* d_bits,
                     hipStream_t s, uint32_t* out_flags) {
  const size_t npix = e->n * count, C = (size_t)e->ch, offb = e->n * (size_t)first * C;
  const size_t slab = e->n * slab_count;  // pixels from one frame of the clip to the next
  const size_t words = slab / 64;
  const Family& fam = *e->fam;
  const bool fuse_ok = e->knob.clip_fuse && fam.clip_fused && (!fam.clip_fusable || fam.clip_fusable(e));
  // FrameDifference / WeightedMoving*: frame t needs frames t-1 (t-2).  A per-frame call copies its frame into the engine's ring; inside
  // a clip the earlier frames of the clip ARE that history, so only the last one (two) are copied into the ring, once, at the end.
  FrameHistory& h = e->hist;
  const bool ring_clip = h.nring > 0 && h.mode == FrameHistory::kPrivate && nframes >= 2;
  const int64_t t0 = e->seen[first], p0 = e->rpos[first];
  std::optional<FrameHistory::Scope> lend;
  if (ring_clip) lend.emplace(h, h.prev(p0, t0, 1, offb), h.prev(p0, t0, 2, offb));
  auto end_ring_clip = [&](int done) -> int {  // `done` frames of the clip went through: leave the ring as per-frame calls would have
    HistoryCopy plan[2];
    const int copies = ring_clip ? history_clip_plan(h.nring, p0, done, plan) : 0;
    for (int i = 0; i < copies; ++i) HIP_TRY(hipMemcpyAsync(h.slot[plan[i].slot] + offb, d_frames + (size_t)plan[i].frame * slab * C, npix * C, hipMemcpyDeviceToDevice, s));
    return BGS_OK;
  };
  for (int t = 0, fuse; t < nframes; t += fuse) {
    const int left = nframes - t;
    fuse = !fuse_ok ? 1 : left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1;
    const uint8_t* fr = d_frames + (size_t)t * slab * C;
    uint8_t* fg = d_fg ? d_fg + (size_t)t * slab : nullptr;
    uint8_t* bg = d_bg ? d_bg + (size_t)t * slab * (size_t)bg_channels(e) : nullptr;
    uint64_t* bits = d_bits ? d_bits + (size_t)t * words : nullptr;
    uint32_t* fl = out_flags ? out_flags + t : nullptr;
    const int rc = fuse == 1 ? process_range(e, first, count, fr, fg, bg, bits, s, fl) : clip_fused_run(e, first, count, fuse, slab, fr, fg, bg, bits, s, fl);
    if (rc) {
      (void)end_ring_clip(t);
      return rc;
    }
  }
  return end_ring_clip(nframes);
}

}  // namespace

// N3 (bgs_ingest_*, bgs_set_ingest): geometry of the frame preparation
namespace {
struct IngestPlan {
  int rw, rh, rows, cols, x0, y0, mode;
  double scale_x, scale_y;
};
int ingest_plan(const bgs_ingest* c, int src_rows, int src_cols, IngestPlan* pl) {
  if (!c || c->struct_size != sizeof(bgs_ingest)) return fail(BGS_ERR_INVALID, "bgs_ingest.struct_size mismatch");
  if (src_rows <= 0 || src_cols <= 0 || c->resize_percent <= 0) return fail(BGS_ERR_INVALID, "bad ingest geometry");
  pl->rw = (int)(((int64_t)src_cols * c->resize_percent) / 100), pl->rh = (int)(((int64_t)src_rows * c->resize_percent) / 100);  // VideoCapture.cpp:142
  if (pl->rw < 1 || pl->rh < 1) return fail(BGS_ERR_INVALID, "resize to %d %% leaves no pixels", c->resize_percent);
  const bool roi = c->roi_x1 > c->roi_x0 && c->roi_y1 > c->roi_y0;
  pl->x0 = roi ? c->roi_x0 : 0, pl->y0 = roi ? c->roi_y0 : 0;
  pl->cols = roi ? c->roi_x1 - c->roi_x0 : pl->rw, pl->rows = roi ? c->roi_y1 - c->roi_y0 : pl->rh;
  if (pl->x0 < 0 || pl->y0 < 0 || pl->x0 + pl->cols > pl->rw || pl->y0 + pl->rows > pl->rh)
    return fail(BGS_ERR_INVALID, "ROI (%d,%d)-(%d,%d) outside the %dx%d frame (cvSetImageROI would fail)", c->roi_x0, c->roi_y0, c->roi_x1, c->roi_y1, pl->rw, pl->rh);
  pl->scale_x = 1. / ((double)pl->rw / src_cols), pl->scale_y = 1. / ((double)pl->rh / src_rows);
  const int isx = (int)std::lrint(pl->scale_x), isy = (int)std::lrint(pl->scale_y);
  const bool area_fast = std::fabs(pl->scale_x - isx) < 2.220446049250313e-16 && std::fabs(pl->scale_y - isy) < 2.220446049250313e-16;
  pl->mode = (pl->rw == src_cols && pl->rh == src_rows) ? 0 : (area_fast && isx == 2 && isy == 2) ? 2 : 1;
  return BGS_OK;
}
// cv::getGaussianKernel(7, 1.5, CV_32F) -> the integer kernel of the 8-bit fixed-point filter (R3, kernel_ingest.h)
void gaussian7_kernel(int ik[7]) {
  float cf[7];
  gaussian_kernel_f32(7, 1.5, cf);
  for (int i = 0; i < 7; ++i) ik[i] = (int)std::lrintf(cf[i] * 256.f);
}
}  // namespace

struct bgs_multicue : McModel {};  // include/bgs_hip.h

extern "C" {

int bgs_abi_version(void) { return BGS_ABI_VERSION; }

const char* bgs_last_error(void) { return g_err.c_str(); }

int bgs_default_params(bgs_algo algo, bgs_params* p) {
  if (!p) return fail(BGS_ERR_INVALID, "params is NULL");
  if (!BGS_ALGO_KNOWN(algo)) return fail(BGS_ERR_INVALID, "unknown algorithm %d", (int)algo);
  std::memset(p, 0, sizeof(*p));
  p->struct_size = (uint32_t)sizeof(*p);
  p->enable_threshold = 1;
  p->threshold = (algo == BGS_ASBL) ? 25 : 15;
  p->enable_weight = 1;
  p->alpha = 0.05;
  p->limit = -1;
  p->learning_frames = 90;
  p->alpha_learn = 0.05;
  p->alpha_detection = 0.05;
  p->mog2_history = 500;
  p->mog2_nmixtures = 5;
  p->mog2_var_threshold = 16.f;
  p->mog2_background_ratio = 0.9f;
  p->mog2_var_threshold_gen = 9.f;
  p->mog2_var_init = 15.f;
  p->mog2_var_min = 4.f;
  p->mog2_var_max = 75.f;
  p->mog2_ct = 0.05f;
  p->mog2_tau = 0.5f;
  p->mog2_detect_shadows = 1;
  p->mog2_shadow_value = 127;
  p->mog1_history = 200;
  p->mog1_nmixtures = 5;
  p->mog1_background_ratio = 0.7;
  p->mog1_var_threshold = 2.5 * 2.5;
  p->mog1_noise_sigma = 30 * 0.5;
  p->lbsp_rel_threshold = 0.333f;
  p->lbsp_threshold_offset = 0;
  p->subsense_min_color_dist_threshold = 30;
  p->subsense_n_samples = 50;
  p->subsense_n_required = 2;
  p->subsense_samples_for_moving_avgs = 100;
  p->subsense_desc_dist_threshold_offset = 3;
  p->gmg_max_features = 64;
  p->gmg_init_frames = 20;
  p->gmg_quantization_levels = 16;
  p->gmg_smoothing_radius = 7;
  p->gmg_update_background_model = 1;
  p->gmg_learning_rate = 0.025;
  p->gmg_background_prior = 0.8;
  p->gmg_decision_threshold = 0.7;
  p->sd_amp_factor = 1;
  p->sd_min_var = 15;
  p->sd_max_var = 255;
  // package_bgs/dp wrappers, DP*BGS.cpp:19
  p->dp_gaussians = 3;
  p->dp_sampling_rate = 7;
  switch (algo) {
    case BGS_DP_ZIVKOVIC_AGMM: p->dp_threshold = 25.0f, p->dp_alpha = 0.001f; break;
    case BGS_DP_GRIMSON_GMM: p->dp_threshold = 9.0f, p->dp_alpha = 0.01f; break;
    case BGS_DP_WREN_GA: p->dp_threshold = 12.25f, p->dp_alpha = 0.005f, p->learning_frames = 30; break;
    case BGS_DP_MEAN: p->dp_threshold = 2700.0f, p->dp_alpha = 1e-6f, p->learning_frames = 30; break;
    case BGS_DP_ADAPTIVE_MEDIAN: p->dp_threshold = 40.0f, p->learning_frames = 30; break;
    case BGS_LOBSTER:  // BackgroundSubtractorLOBSTER.h:6-16
      p->lbsp_rel_threshold = 0.365f, p->subsense_desc_dist_threshold_offset = 4, p->subsense_min_color_dist_threshold = 30;
      p->subsense_n_samples = 35, p->subsense_n_required = 2;
      break;
    case BGS_KDE:  // KDE.cpp:19-20, :114-126 (the kde_* fields stay zero for every other algorithm)
      p->kde_frames_to_learn = 10, p->kde_sequence_length = 50, p->kde_time_window = 100;
      p->kde_sd_estimation = 1, p->kde_color_ratios = 1, p->kde_update_model = 1;
      p->kde_threshold = 10e-8, p->kde_alpha = 0.3;
      break;
    case BGS_DP_PRATI_MEDIOD:  // DPPratiMediodBGS.cpp:19, :98-104 (dp_history_size / dp_weight stay zero for every other algorithm)
      p->dp_threshold = 30.0f, p->dp_sampling_rate = 5, p->dp_history_size = 16, p->dp_weight = 5;
      break;
    // package_bgs/lb wrappers, LB*.cpp:19-20 (the lb_* fields stay zero for every other algorithm)
    case BGS_LB_SIMPLE_GAUSSIAN: p->lb_sensitivity = 66, p->lb_noise_variance = 162, p->lb_learning_rate = 18; break;
    case BGS_LB_FUZZY_GAUSSIAN: p->lb_sensitivity = 72, p->lb_bg_threshold = 162, p->lb_learning_rate = 49, p->lb_noise_variance = 195; break;
    case BGS_LB_MOG: p->lb_sensitivity = 81, p->lb_bg_threshold = 83, p->lb_learning_rate = 59, p->lb_noise_variance = 206; break;
    case BGS_LB_ADAPTIVE_SOM:
      p->lb_sensitivity = 75, p->lb_training_sensitivity = 245, p->lb_learning_rate = 62, p->lb_training_learning_rate = 255, p->lb_training_steps = 55;
      break;
    case BGS_LB_FUZZY_ADAPTIVE_SOM:
      p->lb_sensitivity = 90, p->lb_training_sensitivity = 240, p->lb_learning_rate = 38, p->lb_training_learning_rate = 255, p->lb_training_steps = 81;
      break;
    case BGS_VUMETER:  // VuMeter.cpp:19, :103-116 (the vu_* fields stay zero for every other algorithm)
      p->vu_bin_size = 8, p->vu_enable_filter = 1, p->vu_alpha = 0.995, p->vu_threshold = 0.03;
      break;
    default: break;
  }
  return BGS_OK;
}

int bgs_create(bgs_algo algo, const bgs_params* params, int hip_device, int n_streams, bgs_engine** out) {
  if (!out) return fail(BGS_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!BGS_ALGO_KNOWN(algo)) return fail(BGS_ERR_INVALID, "unknown algorithm %d", (int)algo);
  if (n_streams < 1) return fail(BGS_ERR_INVALID, "n_streams must be >= 1");
  if (params && params->struct_size != sizeof(bgs_params)) return fail(BGS_ERR_INVALID, "bgs_params.struct_size %u != %zu (ABI mismatch)", params->struct_size, sizeof(bgs_params));
  bgs_engine* e = new (std::nothrow) bgs_engine();
  if (!e) return fail(BGS_ERR_NOMEM, "out of host memory");
  e->algo = algo, e->fam = family_of(algo);
  if (params)
    e->p = *params;
  else
    bgs_default_params(algo, &e->p);
  int rc = check_params(algo, e->p);
  if (rc) {
    delete e;
    return rc;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    delete e;
    return fail(BGS_ERR_HIP, "no HIP device visible: libbgs_hip has no CPU path");
  }
  if (hip_device < 0 || hip_device >= ndev) {
    delete e;
    return fail(BGS_ERR_INVALID, "hip_device %d outside 0..%d", hip_device, ndev - 1);
  }
  e->device = hip_device;
  e->S = n_streams;
  e->seen.assign(n_streams, 0);
  e->rpos.assign(n_streams, 0);
  e->host.set_streams(n_streams);
  e->last_flags.assign(n_streams, 0);
  e->counter.assign(n_streams, 0);
  for_each_block([e](const auto& b) { b.defaults(&(e->*b.member)); });  // a class with a block of its own starts from the constructor's values whatever bgs_params it was handed
  if (const char* env = getenv("BGS_KDE_TRIPS")) e->knob.kde_count_trips = atoi(env) != 0;
  if (const char* env = getenv("BGS_MOG2_COMPLETE")) e->knob.mog2_complete = atoi(env) != 0;
  if (const char* env = getenv("BGS_LB_PX")) e->knob.lb_px = atoi(env) == 2 ? 2 : 1;
  if (const char* env = getenv("BGS_VU_SPARSE")) e->knob.vu_sparse = std::min(std::max(atoi(env), 0), 2);
  if (const char* env = getenv("BGS_XCD_SWIZZLE")) e->knob.xcd_swizzle = atoi(env);
  if (const char* env = getenv("BGS_MOG2_SPARSE")) e->knob.mog2_sparse = atoi(env);
  if (const char* env = getenv("BGS_MODEL_CHUNK_MB")) e->knob.model_chunk_mb = atoi(env);
  if (const char* env = getenv("BGS_MODEL_CHUNK_MIN_MB")) e->knob.model_chunk_min_bytes = (size_t)std::max(atoi(env), 0) << 20;
  if (const char* env = getenv("BGS_CLIP_FUSE")) e->knob.clip_fuse = atoi(env) != 0;
  if (const char* env = getenv("BGS_DEBUG_POISON")) e->knob.poison = atoi(env) != 0;
  if (const char* env = getenv("BGS_HOST_REGISTER")) e->knob.host_register = atoi(env) & 7;
  *out = e;
  return BGS_OK;
}

int bgs_set_params(bgs_engine* e, const bgs_params* params) {
  if (!e || !params) return fail(BGS_ERR_INVALID, "NULL argument");
  if (params->struct_size != sizeof(bgs_params)) return fail(BGS_ERR_INVALID, "bgs_params.struct_size mismatch");
  int rc = check_params(e->algo, *params);
  if (rc) return rc;
  const bgs_params old = e->p;
  e->p = *params;
  if (e->n) {
    // Parameters the reference hands to its model object once, when it is built on the first frame, stay as they were:
    // later values are ignored there too (SuBSENSE.cpp:27-36, LOBSTER.cpp:27-34, DP*BGS.cpp `if(firstTime)`), and here they
    // also size the device buffers.
    if (e->fam->keep_frozen) e->fam->keep_frozen(e->p, old);
    if (e->fam->apply_params) return e->fam->apply_params(e);
  }
  return BGS_OK;
}

// The class parameter blocks: each entry point names its block (ParamBlock, block_*).
int bgs_fuzzy_default_params(bgs_fuzzy_params* p) { return block_default(kFuzzyBlock, p); }
int bgs_set_fuzzy_params(bgs_engine* e, const bgs_fuzzy_params* p) { return block_set(kFuzzyBlock, __func__, e, p); }
int bgs_get_fuzzy_params(const bgs_engine* e, bgs_fuzzy_params* p) { return block_get(kFuzzyBlock, __func__, e, p); }
int bgs_fuzzy_check(bgs_algo algo, const bgs_fuzzy_params* p, int rows, int cols, int channels) { return block_check(kFuzzyBlock, __func__, algo, p, rows, cols, channels); }

int bgs_t2f_default_params(bgs_t2f_params* p) { return block_default(kT2fBlock, p); }
int bgs_set_t2f_params(bgs_engine* e, const bgs_t2f_params* p) { return block_set(kT2fBlock, __func__, e, p); }
int bgs_get_t2f_params(const bgs_engine* e, bgs_t2f_params* p) { return block_get(kT2fBlock, __func__, e, p); }
int bgs_t2f_check(bgs_algo algo, const bgs_t2f_params* p, int rows, int cols, int channels) { return block_check(kT2fBlock, __func__, algo, p, rows, cols, channels); }

int bgs_eigen_default_params(bgs_eigen_params* p) { return block_default(kEigenBlock, p); }
int bgs_set_eigen_params(bgs_engine* e, const bgs_eigen_params* p) { return block_set(kEigenBlock, __func__, e, p); }
int bgs_get_eigen_params(const bgs_engine* e, bgs_eigen_params* p) { return block_get(kEigenBlock, __func__, e, p); }
int bgs_eigen_check(const bgs_eigen_params* p, int rows, int cols, int channels) { return block_check(kEigenBlock, __func__, BGS_DP_EIGENBACKGROUND, p, rows, cols, channels); }

int bgs_imbs_default_params(bgs_imbs_params* p) { return block_default(kImbsBlock, p); }
int bgs_set_imbs_params(bgs_engine* e, const bgs_imbs_params* p) { return block_set(kImbsBlock, __func__, e, p); }
int bgs_get_imbs_params(const bgs_engine* e, bgs_imbs_params* p) { return block_get(kImbsBlock, __func__, e, p); }
int bgs_imbs_check(const bgs_imbs_params* p, int rows, int cols, int channels) { return block_check(kImbsBlock, __func__, BGS_IMBS, p, rows, cols, channels); }

int bgs_multilayer_default_params(bgs_multilayer_params* p) { return block_default(kMultilayerBlock, p); }
int bgs_set_multilayer_params(bgs_engine* e, const bgs_multilayer_params* p) { return block_set(kMultilayerBlock, __func__, e, p); }
int bgs_get_multilayer_params(const bgs_engine* e, bgs_multilayer_params* p) { return block_get(kMultilayerBlock, __func__, e, p); }
int bgs_multilayer_check(const bgs_multilayer_params* p, int rows, int cols, int channels) { return block_check(kMultilayerBlock, __func__, BGS_MULTILAYER, p, rows, cols, channels); }

int bgs_multilayer_constants(const bgs_multilayer_params* p, uint32_t bits[2]) {
  if (!bits) return fail(BGS_ERR_INVALID, "NULL argument");
  bgs_multilayer_params d;
  p = block_arg(kMultilayerBlock, p, d);
  if (!p) return BGS_ERR_INVALID;
  const float sine = ml_min_sine(), angle = p->min_noised_angle;
  std::memcpy(&bits[0], &sine, 4), std::memcpy(&bits[1], &angle, 4);
  return BGS_OK;
}

int bgs_set_geometry(bgs_engine* e, int rows, int cols, int channels) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (e->n) {
    if (rows == e->rows && cols == e->cols && channels == e->ch) return BGS_OK;
    return fail(BGS_ERR_GEOMETRY, "engine is %dx%dx%d, asked for %dx%dx%d", e->rows, e->cols, e->ch, rows, cols, channels);
  }
  int rc = allocate(e, rows, cols, channels);
  if (rc) {
    free_all(e);
    e->n = 0;
  }
  return rc;
}

// option 1: borrow the caller's frame buffers as history (device path of FD/WMM/WMV): the buffers passed to the
// previous one (FD) or two (WMM/WMV) bgs_process_batch_device calls must stay valid and unchanged.
int bgs_set_option(bgs_engine* e, int option, int64_t value) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  switch (option) {
    case 1: e->hist.mode = value ? FrameHistory::kBorrowed : FrameHistory::kPrivate; return BGS_OK;
    case 2:  // round-2 A/B knobs (pixels per lane, planar layout): accepted and ignored since the slot layout of round 3
    case 3: return BGS_OK;
    case 4: e->knob.xcd_swizzle = (int)std::min<int64_t>(std::max<int64_t>(value, 0), 2); return BGS_OK;
    case 6: e->knob.mog2_sparse = (int)std::min<int64_t>(std::max<int64_t>(value, 0), 4); return BGS_OK;
    case 7: e->knob.clip_fuse = value != 0; return BGS_OK;
    case 8:
      if (hipSetDevice(e->device) == hipSuccess && e->stream()) (void)hipStreamSynchronize(e->stream());
      (void)hipDeviceSynchronize();
      e->host.unpin_roles_outside((int)(value & 7));
      e->knob.host_register = (int)(value & 7);
      return BGS_OK;
    case 5: return BGS_OK;  // BGS_OPT_PLACEMENT_PROBE of rounds 1-2: accepted and ignored (placement is deterministic since round 3: model_allocate)
    case 9:
      if (e->n) return fail(BGS_ERR_INVALID, "the model is allocated when the geometry is set");
      e->knob.model_chunk_mb = (int)std::max<int64_t>(value, 0);
      return BGS_OK;
    case 10:
      if (e->n) return fail(BGS_ERR_INVALID, "the model is allocated when the geometry is set");
      e->knob.model_chunk_min_bytes = (size_t)std::max<int64_t>(value, 0) << 20;
      return BGS_OK;
    default: return fail(BGS_ERR_INVALID, "unknown option %d", option);
  }
}

// A bgs_submit still in flight runs on its lane's own non-blocking HIP stream: a device-path call over the same camera would race
// with it on that camera's model, ring slot and frame count.  The device entry points refuse instead (bgs_wait first).
static int range_busy(const bgs_engine* e, int first, int count) {
  for (int i = std::max(first, 0); i < first + count && i < e->S; ++i)
    if (e->host.sub[i].pending) return fail(BGS_ERR_STATE, "stream %d has a bgs_submit in flight: bgs_wait before a device-path call that covers it", i);
  return BGS_OK;
}

int bgs_process_range_device(bgs_engine* e, int first, int count, const void* d_frames, void* d_fg, void* d_bg, void* d_fg_bits, void* hip_stream,
                             uint32_t* out_flags) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (int rc = range_busy(e, first, count)) return rc;
  return process_range(e, first, count, (const uint8_t*)d_frames, (uint8_t*)d_fg, (uint8_t*)d_bg, (uint64_t*)d_fg_bits, (hipStream_t)hip_stream, out_flags);
}

int bgs_process_clip_device(bgs_engine* e, int first, int count, int nframes, const void* d_frames, void* d_fg, void* d_bg, void* d_fg_bits,
                            void* hip_stream, uint32_t* out_flags) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (int rc = range_busy(e, first, count)) return rc;
  return process_clip(e, first, count, nframes, (const uint8_t*)d_frames, (uint8_t*)d_fg, (uint8_t*)d_bg, (uint64_t*)d_fg_bits, (hipStream_t)hip_stream, out_flags);
}

int bgs_process_batch_device(bgs_engine* e, const void* d_frames, void* d_fg, void* d_bg, void* d_fg_bits, void* hip_stream, uint32_t* out_flags) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (int rc = range_busy(e, 0, e->S)) return rc;
  return process_range(e, 0, e->S, (const uint8_t*)d_frames, (uint8_t*)d_fg, (uint8_t*)d_bg, (uint64_t*)d_fg_bits, (hipStream_t)hip_stream, out_flags);
}

static int lane_wait(bgs_engine* e, int stream, uint32_t* out_flags);  // bgs_submit / bgs_wait, below

// where the frame of a host call goes on the device: the history classes receive the upload straight in their ring slot (zero-copy history)
static uint8_t* lane_dst(const bgs_engine* e, const Lane& ln, int stream) {
  uint8_t* slot = e->hist.keep_at(e->rpos[stream], (size_t)stream * e->n * e->ch);
  return slot ? slot : ln.in.d;
}

// What bgs_process and bgs_submit do with a frame on their lane: the upload - straight from the caller's page-locked buffer, or staged
// (map: bgs_set_ingest's flip / ROI, free of charge: the row map says where each staged row starts); not when the ingest kernels wrote
// the frame (in == NULL) - then the model's step with private history.  The mask stays on the device for bgs_last_mask_blobs.
static int lane_frame(bgs_engine* e, Lane& ln, int stream, const uint8_t* in, size_t in_step, const RowMap* map, bool want_bg, uint32_t* flags) {
  HostPath& hp = e->host;
  const size_t rb = (size_t)e->cols * e->ch, fb = e->n * e->ch;
  uint8_t* dst = lane_dst(e, ln, stream);
  if (in) {
    hp.frames++, hp.h2d_bytes += (int64_t)fb;
    if (!map && in_step == rb && host_pin(e, stream, 0, in, fb, ln.hs)) {
      HIP_TRY(hipMemcpyAsync(dst, in, fb, hipMemcpyHostToDevice, ln.hs));
    } else {
      const auto st0 = std::chrono::steady_clock::now();
      HIP_TRY(upload_rows(ln.in, dst, ln.hs, in, in_step, rb, e->rows, band_count(e->rows), map));
      hp.stage_in_ms += ms_since(st0);
    }
  }
  FrameHistory::Scope own(e->hist);
  return process_range(e, stream, 1, dst, ln.fg.d, want_bg ? ln.bg.d : nullptr, nullptr, ln.hs, flags);
}

int bgs_process(bgs_engine* e, int stream, const uint8_t* in, int rows, int cols, int channels, size_t in_step, uint8_t* fg, size_t fg_step, uint8_t* bg,
                size_t bg_step, uint32_t* out_flags) {
  if (out_flags) *out_flags = 0;
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (stream < 0 || stream >= e->S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, e->S - 1);
  if (!in || rows <= 0 || cols <= 0) return BGS_OK;  // if(img_input.empty()) return;
  if (channels != 1 && channels != 3) return fail(BGS_ERR_UNSUPPORTED, "channels must be 1 or 3");
  if (in_step < (size_t)cols * channels) return fail(BGS_ERR_INVALID, "in_step %zu < cols*channels", in_step);
  // N3: with bgs_set_ingest the caller hands over the RAW captured frame; everything below runs in the prepared geometry
  IngestPlan pl{};
  const bool ingest = e->ingest_on;
  const int raw_rows = rows, raw_cols = cols;
  if (ingest) {
    int rc0 = ingest_plan(&e->ingest, rows, cols, &pl);
    if (rc0) return rc0;
    if (e->ingest.equalize_hist && channels != 1) return fail(BGS_ERR_UNSUPPORTED, "equalizeHist needs a 1-channel frame (cv::equalizeHist asserts CV_8UC1, PreProcessor.cpp:64)");
    if (e->raw_rows && (e->raw_rows != rows || e->raw_cols != cols)) return fail(BGS_ERR_GEOMETRY, "raw frames were %dx%d, now %dx%d", e->raw_rows, e->raw_cols, rows, cols);
    e->raw_rows = rows, e->raw_cols = cols;
    rows = pl.rows, cols = pl.cols;
  }
  const bool ingest_on_device = ingest && (pl.mode != 0 || e->ingest.equalize_hist || e->ingest.gaussian_blur);
  int rc = bgs_set_geometry(e, rows, cols, channels);
  if (rc) return rc;
  HostPath& hp = e->host;
  Lane& ln = hp.sync;
  if (hp.sub[stream].pending) {  // a bgs_submit of this stream is still in flight: its result is collected (and dropped) first
    rc = lane_wait(e, stream, nullptr);
    if (rc) return rc;
  }
  rc = lane_make(e, ln, "bgs_process", stream);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (ingest_on_device) {
    // resize / equalizeHist / GaussianBlur: the raw frame goes up as it is, the preparation runs between the upload and the model kernel
    const size_t raw_rb = (size_t)raw_cols * channels;
    if (!hp.raw.h) {  // with its workspace, or not at all
      hipError_t er = hp.ingest_ws.make(bgs_ingest_workspace(&e->ingest, 1, raw_rows, raw_cols, channels), /*host=*/false);
      if (er == hipSuccess && (er = hp.raw.make(raw_rb * raw_rows)) != hipSuccess) hp.ingest_ws.release();
      if (er != hipSuccess) return fail(BGS_ERR_HIP, "bgs_process: staging of the raw frame: %s", hipGetErrorString(er));
    }
    HIP_TRY(upload_rows(hp.raw, hp.raw.d, ln.hs, in, in_step, raw_rb, raw_rows, band_count(raw_rows)));
    rc = bgs_ingest_device(e->device, &e->ingest, hp.raw.d, 1, raw_rows, raw_cols, channels, raw_rb, lane_dst(e, ln, stream), hp.ingest_ws.d, ln.hs);
    if (rc) return rc;
  }
  uint32_t flags = 0;
  const RowMap map{e->ingest.flip != 0, pl.rh, pl.y0, (size_t)pl.x0 * channels};
  e->last_fg_stream = -1;
  rc = lane_frame(e, ln, stream, ingest_on_device ? nullptr : in, in_step, ingest ? &map : nullptr, bg != nullptr, &flags);
  if (rc) return rc;
  if (flags & BGS_FG_VALID) e->last_fg_stream = stream;
  const int bg_ch = bg_channels(e);
  // the way back is banded when there is a background image to return (6 MB at 1080p); a mask alone (2 MB) is not worth the events
  bool out_fg = fg && (flags & BGS_FG_VALID), out_bg = bg && (flags & BGS_BG_VALID);
  // outputs the caller keeps allocated (same buffer as last call, contiguous rows) are written by the DMA engine directly
  const bool fg_direct = out_fg && fg_step == (size_t)cols && host_pin(e, stream, 1, fg, e->n, ln.hs);
  const bool bg_direct = out_bg && bg_step == (size_t)cols * bg_ch && host_pin(e, stream, 2, bg, e->n * bg_ch, ln.hs);
  hp.d2h_bytes += (int64_t)((out_fg ? e->n : 0) + (out_bg ? e->n * bg_ch : 0));
  if (fg_direct) HIP_TRY(hipMemcpyAsync(fg, ln.fg.d, e->n, hipMemcpyDeviceToHost, ln.hs));
  if (bg_direct) HIP_TRY(hipMemcpyAsync(bg, ln.bg.d, e->n * bg_ch, hipMemcpyDeviceToHost, ln.hs));
  if (fg_direct) out_fg = false;
  if (bg_direct) out_bg = false;
  if (!out_fg && !out_bg)
    HIP_TRY(hipStreamSynchronize(ln.hs));
  else
    HIP_TRY(ln.download_banded(rows, out_bg ? band_count(rows) : 1, {&ln.fg, out_fg ? fg : nullptr, fg_step, (size_t)cols}, {&ln.bg, out_bg ? bg : nullptr, bg_step, (size_t)cols * bg_ch}));
  if (out_flags) *out_flags = flags;
  return BGS_OK;
}

// ---- several cameras on the host path: bgs_submit queues one frame of one stream and returns, bgs_wait collects it ----------
// Each camera has its own lane (HIP stream, pinned staging, device images), so while camera A's frame is on the bus camera B's
// kernel runs and camera C's mask comes back: the copy engines and the CUs work side by side instead of taking turns, which is all
// a synchronous bgs_process per camera can do.  One submission per stream in flight; bgs_process on a stream first collects it.
static int lane_wait(bgs_engine* e, int stream, uint32_t* out_flags) {
  const Lane& ln = e->host.lanes[stream];
  HostPath::Submission& sub = e->host.sub[stream];
  if (out_flags) *out_flags = 0;
  if (!sub.pending) return BGS_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipEventSynchronize(ln.done));
  sub.pending = false;
  const bool copy_fg = sub.fg && !sub.fg_direct && (sub.flags & BGS_FG_VALID), copy_bg = sub.bg && !sub.bg_direct && (sub.flags & BGS_BG_VALID);
  const auto st0 = std::chrono::steady_clock::now();
  if (copy_fg) unpack_rows(sub.fg, sub.fg_step, ln.fg.h, (size_t)e->cols, 0, e->rows);
  if (copy_bg) unpack_rows(sub.bg, sub.bg_step, ln.bg.h, (size_t)e->cols * bg_channels(e), 0, e->rows);
  if (copy_fg || copy_bg) e->host.stage_out_ms += ms_since(st0);
  if (out_flags) *out_flags = sub.flags;
  return BGS_OK;
}

int bgs_submit(bgs_engine* e, int stream, const uint8_t* in, int rows, int cols, int channels, size_t in_step, uint8_t* fg, size_t fg_step, uint8_t* bg,
               size_t bg_step) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (stream < 0 || stream >= e->S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, e->S - 1);
  if (e->ingest_on) return fail(BGS_ERR_UNSUPPORTED, "bgs_submit takes prepared frames (bgs_set_ingest is served by bgs_process)");
  if (e->host.sub[stream].pending) return fail(BGS_ERR_STATE, "stream %d has a submission in flight: bgs_wait first", stream);
  if (!in || rows <= 0 || cols <= 0) return BGS_OK;  // if(img_input.empty()) return;
  if (channels != 1 && channels != 3) return fail(BGS_ERR_UNSUPPORTED, "channels must be 1 or 3");
  if (in_step < (size_t)cols * channels) return fail(BGS_ERR_INVALID, "in_step %zu < cols*channels", in_step);
  int rc = bgs_set_geometry(e, rows, cols, channels);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));
  HostPath& hp = e->host;
  Lane& ln = hp.lanes[stream];
  HostPath::Submission& sub = hp.sub[stream];
  const int bg_ch = bg_channels(e);
  rc = lane_make(e, ln, "bgs_submit", stream);
  if (rc) return rc;
  uint32_t flags = 0;
  if (e->last_fg_stream == stream) e->last_fg_stream = -1;  // bgs_last_mask_blobs serves the synchronous call's mask
  rc = lane_frame(e, ln, stream, in, in_step, nullptr, bg != nullptr, &flags);
  if (rc) return rc;
  const bool out_fg = fg && (flags & BGS_FG_VALID), out_bg = bg && (flags & BGS_BG_VALID);
  sub.flags = flags, sub.fg = fg, sub.bg = bg, sub.fg_step = fg_step, sub.bg_step = bg_step;
  sub.fg_direct = out_fg && fg_step == (size_t)cols && host_pin(e, stream, 1, fg, e->n, ln.hs);
  sub.bg_direct = out_bg && bg_step == (size_t)cols * bg_ch && host_pin(e, stream, 2, bg, e->n * bg_ch, ln.hs);
  hp.d2h_bytes += (int64_t)((out_fg ? e->n : 0) + (out_bg ? e->n * bg_ch : 0));
  if (out_fg) HIP_TRY(sub.fg_direct ? hipMemcpyAsync(fg, ln.fg.d, e->n, hipMemcpyDeviceToHost, ln.hs) : download_whole(ln.fg, e->n, ln.hs));
  if (out_bg) HIP_TRY(sub.bg_direct ? hipMemcpyAsync(bg, ln.bg.d, e->n * bg_ch, hipMemcpyDeviceToHost, ln.hs) : download_whole(ln.bg, e->n * bg_ch, ln.hs));
  HIP_TRY(hipEventRecord(ln.done, ln.hs));
  sub.pending = true;
  return BGS_OK;
}

int bgs_host_arena(bgs_engine* e, void* ptr, size_t bytes, int on) {
  if (!e || !ptr || (on && !bytes)) return fail(BGS_ERR_INVALID, "bgs_host_arena: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  auto& arenas = e->host.arenas;
  for (size_t i = 0; i < arenas.size(); ++i)
    if (arenas[i].first == (const uint8_t*)ptr) {
      if (on) return arenas[i].second == bytes ? BGS_OK : fail(BGS_ERR_INVALID, "bgs_host_arena: this address is registered with another size");
      (void)hipDeviceSynchronize();  // nothing may still be reading or writing it
      HIP_TRY(hipHostUnregister(ptr));
      e->host.unreg_calls++;
      arenas.erase(arenas.begin() + (long)i);
      return BGS_OK;
    }
  if (!on) return fail(BGS_ERR_INVALID, "bgs_host_arena: no such arena");
  const hipError_t er = e->host.timed_register(ptr, bytes);
  if (er != hipSuccess) return fail(BGS_ERR_HIP, "hipHostRegister of a %zu-byte arena failed: %s", bytes, hipGetErrorString(er));
  arenas.emplace_back((const uint8_t*)ptr, bytes);
  return BGS_OK;
}

int bgs_wait(bgs_engine* e, int stream, uint32_t* out_flags) {
  if (out_flags) *out_flags = 0;
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (stream < 0 || stream >= e->S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, e->S - 1);
  return lane_wait(e, stream, out_flags);
}

int64_t bgs_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap) {
  if (!e || !plane || !dst) return fail(BGS_ERR_INVALID, "NULL argument");
  if (!e->n) return fail(BGS_ERR_STATE, "no model yet");
  if (stream < 0 || stream >= e->S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, e->S - 1);
  if (hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(BGS_ERR_HIP, "device sync failed");
  if (!strcmp(plane, "hostpath")) {  // diagnostics of bgs_process / bgs_submit since creation: 15 doubles (see bench.py host_path)
    const HostPath& hp = e->host;
    double rec[15] = {0};
    for (size_t i = 0; i < hp.pin.size(); ++i) rec[i % 3] += hp.pin[i].pinned, rec[3 + i % 3] += hp.pin[i].refused;  // per role: input, mask, background
    rec[6] = (double)hp.reg_calls, rec[7] = hp.reg_ms, rec[8] = (double)hp.unreg_calls, rec[9] = (double)hp.frames;
    rec[10] = (double)hp.h2d_bytes, rec[11] = (double)hp.d2h_bytes, rec[12] = hp.stage_in_ms, rec[13] = hp.stage_out_ms, rec[14] = (double)hp.arenas.size();
    return copy_host(plane, dst, cap, rec, sizeof(rec));
  }
  if (!strcmp(plane, "placement")) {  // diagnostics: [0] chunk size in MiB of the chunked model (0: one plain allocation), [1] number of chunks
    float rec[2] = {e->vmm.base ? (float)(e->vmm.chunk >> 20) : 0.f, (float)e->vmm.handles.size()};
    return copy_host(plane, dst, cap, rec, sizeof(rec));
  }
  return e->fam->get_state(e, stream, plane, dst, cap);
}

int64_t bgs_frames_seen(const bgs_engine* e, int stream) {
  if (!e || stream < 0 || stream >= e->S) return BGS_ERR_INVALID;
  return e->seen[stream];
}

// One camera starts over: what deleting its IBGS object and creating a new one does in the reference (FrameProcessor.cpp:342-482 then
// :35-155; ustc_src/ustc_bgs.cpp:75-77).  Nothing is launched here: the stream's frame count goes back to 0, so its next frame - on
// whatever HIP stream that call uses, in order with everything before it - re-initialises its model exactly like a first frame
// (mog2_clear, ss_init_streams, the warm-up of the history classes ...).  The other streams of the batch are not touched and keep
// sharing launches with each other; the reset stream re-joins them as soon as its launch arguments equal theirs again (launch_key).
int bgs_reset_stream(bgs_engine* e, int stream) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (stream < 0 || stream >= e->S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, e->S - 1);
  e->seen[stream] = 0, e->counter[stream] = 0, e->last_flags[stream] = 0;
  if (e->model && e->fam->reset_stream) e->fam->reset_stream(e, stream);
  if (e->last_fg_stream == stream) e->last_fg_stream = -1;
  return BGS_OK;
}

int bgs_stream_flags(const bgs_engine* e, int stream, uint32_t* out_flags) {
  if (!e || !out_flags) return fail(BGS_ERR_INVALID, "NULL argument");
  if (stream < 0 || stream >= e->S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, e->S - 1);
  *out_flags = e->last_flags[stream];
  return BGS_OK;
}

int bgs_enable_kernel_timing(bgs_engine* e, int on) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  e->timer.enable(on != 0);
  return BGS_OK;
}

int bgs_kernel_timing(bgs_engine* e, double* avg_ms, int64_t* launches, const char** kernel_name) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  HIP_TRY(hipSetDevice(e->device));
  double total = 0;
  int64_t n = 0;
  HIP_TRY(e->timer.read(true, INT64_MAX, nullptr, &n, &total));
  if (avg_ms) *avg_ms = n ? total / (double)n : 0.0;
  if (launches) *launches = n;
  if (kernel_name) *kernel_name = e->kernel_name;
  return BGS_OK;
}

int64_t bgs_kernel_timing_series(bgs_engine* e, float* ms, int64_t cap) {
  if (!e || !ms || cap < 0) return fail(BGS_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(e->device));
  double total = 0;
  int64_t n = 0;
  HIP_TRY(e->timer.read(true, cap, ms, &n, &total));
  return n;
}

void bgs_destroy(bgs_engine* e) {
  if (!e) return;
  if (e->n || e->stream()) {
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
  }
  free_all(e);
  delete e;  // ~HostPath closes the engine's stream
}

// ---- measurement aids (bench.py `calibration`): what THIS box's memory system and bus deliver, measured by the library that is being
// benchmarked, in the process that benchmarks it --------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void calib_copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
}  // namespace

int bgs_calibrate_copy(int hip_device, size_t bytes, int chunk_mb, int iters, double* gbps) {
  if (!gbps || bytes < (1u << 20) || iters < 1 || chunk_mb < 0) return fail(BGS_ERR_INVALID, "bgs_calibrate_copy: bad argument");
  *gbps = 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(BGS_ERR_HIP, "no HIP device visible: libbgs_hip has no CPU path");
  HIP_TRY(hipSetDevice(hip_device));
  const size_t half = bytes / 2 / 4096 * 4096, n = half / 16;
  VmmRange v;
  void* base = nullptr;
  if (chunk_mb > 0) {
    if (vmm_allocate(v, hip_device, &base, 2 * half, (size_t)chunk_mb << 20) != BGS_OK) {
      vmm_free(v);
      return BGS_ERR_HIP;  // text set by vmm_allocate
    }
  } else {
    HIP_TRY(hipMalloc(&base, 2 * half));
  }
  hipStream_t s = nullptr;
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t er = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (er == hipSuccess) er = hipEventCreate(&a);
  if (er == hipSuccess) er = hipEventCreate(&b);
  if (er == hipSuccess) er = hipMemsetAsync(base, 1, 2 * half, s);
  float ms = 0;
  if (er == hipSuccess) {
    const dim3 grid((unsigned)((n + 255) / 256));
    for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(calib_copy_kernel, grid, dim3(256), 0, s, (const float4*)base, (float4*)((char*)base + half), n);
    er = hipEventRecord(a, s);
    for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(calib_copy_kernel, grid, dim3(256), 0, s, (const float4*)base, (float4*)((char*)base + half), n);
    if (er == hipSuccess) er = hipEventRecord(b, s);
    if (er == hipSuccess) er = hipEventSynchronize(b);
    if (er == hipSuccess) er = hipEventElapsedTime(&ms, a, b);
    if (er == hipSuccess) er = hipGetLastError();
  }
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
  if (chunk_mb > 0)
    vmm_free(v);
  else
    (void)hipFree(base);
  if (er != hipSuccess) return fail(BGS_ERR_HIP, "bgs_calibrate_copy: %s", hipGetErrorString(er));
  *gbps = ms > 0 ? 2.0 * (double)half * iters / (ms * 1e-3) / 1e9 : 0.0;  // half read + half written per launch
  return BGS_OK;
}

int bgs_calibrate_pcie(int hip_device, size_t bytes, int registered, int iters, double* h2d_gbps, double* d2h_gbps, double* register_ms) {
  if (bytes < 4096 || iters < 1) return fail(BGS_ERR_INVALID, "bgs_calibrate_pcie: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(BGS_ERR_HIP, "no HIP device visible: libbgs_hip has no CPU path");
  HIP_TRY(hipSetDevice(hip_device));
  void *h = nullptr, *d = nullptr;
  double reg = 0;
  if (registered) {  // the caller-buffer case of BGS_OPT_HOST_REGISTER: ordinary pageable memory, page-locked in place
    if (posix_memalign(&h, 4096, bytes)) return fail(BGS_ERR_NOMEM, "out of host memory");
    std::memset(h, 1, bytes);
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t er = hipHostRegister(h, bytes, hipHostRegisterDefault);
    reg = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (er != hipSuccess) {
      free(h);
      return fail(BGS_ERR_HIP, "hipHostRegister failed: %s", hipGetErrorString(er));
    }
  } else {
    HIP_TRY(hipHostMalloc(&h, bytes, hipHostMallocDefault));
    std::memset(h, 1, bytes);
  }
  hipStream_t s = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  hipError_t er = hipMalloc(&d, bytes);
  if (er == hipSuccess) er = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  for (auto& e1 : ev)
    if (er == hipSuccess) er = hipEventCreate(&e1);
  float up = 0, down = 0;
  if (er == hipSuccess) {
    (void)hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s);  // warm
    (void)hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s);
    (void)hipEventRecord(ev[0], s);
    for (int i = 0; i < iters; ++i) (void)hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s);
    (void)hipEventRecord(ev[1], s);
    for (int i = 0; i < iters; ++i) (void)hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s);
    er = hipEventRecord(ev[2], s);
    if (er == hipSuccess) er = hipEventSynchronize(ev[2]);
    if (er == hipSuccess) er = hipEventElapsedTime(&up, ev[0], ev[1]);
    if (er == hipSuccess) er = hipEventElapsedTime(&down, ev[1], ev[2]);
  }
  for (auto& e1 : ev)
    if (e1) (void)hipEventDestroy(e1);
  if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
  if (d) (void)hipFree(d);
  if (registered)
    (void)hipHostUnregister(h), free(h);
  else
    (void)hipHostFree(h);
  if (er != hipSuccess) return fail(BGS_ERR_HIP, "bgs_calibrate_pcie: %s", hipGetErrorString(er));
  if (h2d_gbps) *h2d_gbps = up > 0 ? (double)bytes * iters / (up * 1e-3) / 1e9 : 0.0;
  if (d2h_gbps) *d2h_gbps = down > 0 ? (double)bytes * iters / (down * 1e-3) / 1e9 : 0.0;
  if (register_ms) *register_ms = reg;
  return BGS_OK;
}

int bgs_lbsp_describe_device(int hip_device, const void* d_img, int rows, int cols, int channels, const uint8_t* t_lut, void* d_desc, void* hip_stream) {
  return bgs_lbsp_describe_batch_device(hip_device, d_img, 1, rows, cols, channels, t_lut, d_desc, hip_stream);
}

int bgs_lbsp_describe_batch_device(int hip_device, const void* d_img, int images, int rows, int cols, int channels, const uint8_t* t_lut, void* d_desc,
                                   void* hip_stream) {
  if (!d_img || !d_desc || !t_lut || rows <= 0 || cols <= 0 || images <= 0 || images > 65535) return fail(BGS_ERR_INVALID, "bad argument");
  if (images > 1 && ((size_t)rows * cols * channels) % 4) return fail(BGS_ERR_INVALID, "batched images must each be a multiple of 4 bytes (4-byte aligned rows of dwords)");
  if (channels != 1 && channels != 3) return fail(BGS_ERR_UNSUPPORTED, "channels must be 1 or 3");
  if (!aligned(d_img, 4)) return fail(BGS_ERR_INVALID, "image must be 4-byte aligned");
  HIP_TRY(hipSetDevice(hip_device));
  bgs::LbspArgs a{};
  a.img = (const uint8_t*)d_img, a.desc = (uint16_t*)d_desc, a.rows = rows, a.cols = cols;
  std::memcpy(a.lut, t_lut, 256);
  const dim3 grid((cols + bgs::kLbspTW - 1) / bgs::kLbspTW, (rows + bgs::kLbspTH - 1) / bgs::kLbspTH, images);
  if (channels == 3)
    hipLaunchKernelGGL((bgs::lbsp_kernel<3>), grid, dim3(bgs::kBlock), 0, (hipStream_t)hip_stream, a);
  else
    hipLaunchKernelGGL((bgs::lbsp_kernel<1>), grid, dim3(bgs::kBlock), 0, (hipStream_t)hip_stream, a);
  HIP_TRY(hipGetLastError());
  return BGS_OK;
}

int bgs_mask_morph_device(int hip_device, const void* d_src, void* d_dst, int rows, int cols, int op, int ksize, int iterations, void* hip_stream) {
  if (!d_src || !d_dst || rows <= 0 || cols <= 0 || op < 0 || op > 4 || iterations < 1) return fail(BGS_ERR_INVALID, "bad argument");
  if ((op == 2 || op == 3) && (ksize < 3 || ksize > 2 * bgs::kMorphMaxR + 1 || ksize % 2 == 0)) return fail(BGS_ERR_INVALID, "median ksize must be odd, 3..15");
  if (d_src == d_dst) return fail(BGS_ERR_INVALID, "in-place morphology is not supported");
  HIP_TRY(hipSetDevice(hip_device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (op == 4) {  // cv::floodFill(img, Point(0,0), 255)
    const int W64 = (cols + 63) / 64, tilesY = (rows + 63) / 64;
    uint64_t *mb = nullptr, *rb = nullptr;
    int* fl = nullptr;
    HIP_TRY(hipMalloc((void**)&mb, (size_t)rows * W64 * 8));
    HIP_TRY(hipMalloc((void**)&rb, (size_t)rows * W64 * 8));
    HIP_TRY(hipMalloc((void**)&fl, bgs::kSsFloodFlags * sizeof(int)));
    (void)hipMemsetAsync(fl, 0, bgs::kSsFloodFlags * sizeof(int), s);
    hipLaunchKernelGGL(bgs::ss_flood_pack_kernel, dim3(blocks_for((size_t)rows * W64 * bgs::kWave)), dim3(bgs::kBlock), 0, s, (const uint8_t*)d_src, mb, rb, rows, cols, W64);
    hipLaunchKernelGGL(bgs::ss_flood_seed_kernel, dim3(1), dim3(bgs::kBlock), 0, s, (const uint64_t*)mb, rb, rows, cols, W64);
    // the same host-free sequence as SuBSENSE's post-processing (engine_subsense.h): a fixed batch, then the finish kernel
    for (int k = 0; k < bgs::kSsFloodBatch; ++k) ss_launch_flood(dim3(blocks_for((size_t)tilesY * W64 * bgs::kWave)), 1, tilesY, s, mb, rb, rows, W64, fl, k);
    hipLaunchKernelGGL(bgs::ss_flood_finish_kernel, dim3(1), dim3(1024), 0, s, (const uint64_t*)mb, rb, rows, W64, fl, bgs::kSsFloodBatch);
    hipLaunchKernelGGL(bgs::ss_flood_paint_kernel, dim3(blocks_for((size_t)rows * cols)), dim3(bgs::kBlock), 0, s, (const uint8_t*)d_src, (const uint64_t*)rb, (uint8_t*)d_dst, rows, cols, W64);
    hipError_t er = hipStreamSynchronize(s);
    (void)hipFree(mb), (void)hipFree(rb), (void)hipFree(fl);
    if (er != hipSuccess) return fail(BGS_ERR_HIP, "flood fill failed: %s", hipGetErrorString(er));
    return BGS_OK;
  }
  const size_t n = (size_t)rows * cols;
  // n iterations of the 3x3 erode/dilate are one (2n+1)^2 box (kernel_stencil.h); a launch covers up to kMorphMaxR of them
  int passes = iterations, per_pass = 1;
  if (op <= 1) per_pass = bgs::kMorphMaxR, passes = (iterations + per_pass - 1) / per_pass;
  uint8_t* tmp = nullptr;
  if (passes > 1) HIP_TRY(hipMalloc((void**)&tmp, n));
  const uint8_t* in = (const uint8_t*)d_src;
  int left = iterations;
  for (int i = 0; i < passes; ++i) {
    // alternate so that the last pass lands in d_dst
    uint8_t* out = ((passes - 1 - i) % 2 == 0) ? (uint8_t*)d_dst : tmp;
    const int it = op <= 1 ? std::min(left, per_pass) : 1;
    bgs::MorphArgs a{in, out, rows, cols, op, op <= 1 ? 2 * it + 1 : ksize};
    bgs::morph_launch(a, 1, s);
    left -= it;
    in = out;
  }
  hipError_t er = hipGetLastError();
  if (tmp) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(tmp);
  }
  if (er != hipSuccess) return fail(BGS_ERR_HIP, "morph kernel launch failed: %s", hipGetErrorString(er));
  return BGS_OK;
}

int bgs_canny_device(int hip_device, const void* d_src, void* d_dst, int images, int rows, int cols, int low, int high, void* hip_stream) {
  if (!d_src || !d_dst || images <= 0 || images > 65535 || rows <= 0 || cols <= 0) return fail(BGS_ERR_INVALID, "bgs_canny_device: bad argument");
  if (d_src == d_dst) return fail(BGS_ERR_INVALID, "bgs_canny_device: in-place operation is not supported");
  if ((size_t)rows * cols > (size_t)bgs::kCannyMaxPixels)
    return fail(BGS_ERR_UNSUPPORTED, "bgs_canny_device: %d x %d is more than BGS_CANNY_MAX_PIXELS (%d) pixels", rows, cols, bgs::kCannyMaxPixels);
  static_assert(BGS_CANNY_MAX_PIXELS == bgs::kCannyMaxPixels, "BGS_CANNY_MAX_PIXELS");
  HIP_TRY(hipSetDevice(hip_device));
  if (low > high) std::swap(low, high);  // cvCanny orders its two thresholds itself
  hipLaunchKernelGGL(bgs::canny_kernel, dim3(images), dim3(bgs::kCannyBlock), 0, (hipStream_t)hip_stream, (const uint8_t*)d_src, (uint8_t*)d_dst, rows, cols, low, high);
  HIP_TRY(hipGetLastError());
  return BGS_OK;
}

// ---- the LbpMrf mask stage (gridcut.h)
int bgs_lbpmrf_mask_check(int rows, int cols, int histogram_area, float min_cut_weight) {
  if (histogram_area < 3 || histogram_area % 2 == 0)
    return fail(BGS_ERR_UNSUPPORTED, "LbpMrf: histogram_area %d: it must be odd and at least 3", histogram_area);
  if (!std::isfinite(min_cut_weight)) return fail(BGS_ERR_UNSUPPORTED, "LbpMrf: min_cut_weight is not finite");
  if (rows < histogram_area || cols - histogram_area + 1 < 2)
    return fail(BGS_ERR_UNSUPPORTED, "LbpMrf: a %d x %d frame has no node for histogram_area %d", rows, cols, histogram_area);
  if ((cols - histogram_area + 1) % 2)
    return fail(BGS_ERR_UNSUPPORTED, "LbpMrf: cols - histogram_area + 1 = %d is odd (the reference reads past its node array there)", cols - histogram_area + 1);
  return BGS_OK;
}

namespace {
std::mutex g_lbpmrf_mu;
unsigned long long* g_lbpmrf_stats[64];  // per device: [0] sticky "did not converge" counter, [1] launches of the last call; never freed

int lbpmrf_stats(int hip_device, unsigned long long** out) {
  if (hip_device < 0 || hip_device >= 64) return fail(BGS_ERR_INVALID, "LbpMrf: bad device %d", hip_device);
  std::lock_guard<std::mutex> lock(g_lbpmrf_mu);
  if (!g_lbpmrf_stats[hip_device]) {
    unsigned long long* p = nullptr;
    HIP_TRY(hipMalloc((void**)&p, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(p, 0, 2 * sizeof(unsigned long long)));
    g_lbpmrf_stats[hip_device] = p;
  }
  *out = g_lbpmrf_stats[hip_device];
  return BGS_OK;
}
}  // namespace

int bgs_lbpmrf_mask_counters(int hip_device, uint64_t* not_converged, uint64_t* last_launches) {
  HIP_TRY(hipSetDevice(hip_device));
  unsigned long long* st = nullptr;
  int rc = lbpmrf_stats(hip_device, &st);
  if (rc) return rc;
  unsigned long long h[2];
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h, st, sizeof(h), hipMemcpyDeviceToHost));
  if (not_converged) *not_converged = h[0];
  if (last_launches) *last_launches = h[1];
  return BGS_OK;
}

int bgs_lbpmrf_mask_device(int hip_device, const void* d_rate, void* d_mask, void* d_labels, void* d_flow, int images, int rows, int cols, int histogram_area,
                           float min_cut_weight, void* hip_stream) {
  if (!d_rate || !d_mask || images <= 0 || images > 65535 || rows <= 0 || cols <= 0) return fail(BGS_ERR_INVALID, "bgs_lbpmrf_mask_device: bad argument");
  int rc = bgs_lbpmrf_mask_check(rows, cols, histogram_area, min_cut_weight);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(hip_device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int nh = rows - histogram_area + 1, nw = (cols - histogram_area + 1) / 2;
  const size_t n = (size_t)images * nh * nw, px = (size_t)images * rows * cols;
  if ((size_t)nh * nw > (size_t)INT32_MAX) return fail(BGS_ERR_UNSUPPORTED, "LbpMrf: too many nodes");
  const int W64 = (cols + 63) / 64, tilesY = (rows + 63) / 64, budget = bgs::gc_launch_budget(nh, nw);
  const size_t words = (size_t)images * rows * W64;
  unsigned long long* stats = nullptr;
  if ((rc = lbpmrf_stats(hip_device, &stats))) return rc;
  // one stream-ordered allocation, carved up (256-byte pieces): nothing here waits for the device
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_int = up(n * sizeof(int)), b_ctl = up(bgs::gc_ctl_bytes(budget) + (size_t)images * sizeof(int)), b_lab = d_labels ? 0 : up(n), b_px = up(px),
               b_bits = up(words * 8), b_fl = up((size_t)images * bgs::kSsFloodFlags * sizeof(int));
  char* ws = nullptr;
  HIP_TRY(hipMallocAsync((void**)&ws, 3 * b_int + b_ctl + b_lab + 2 * b_px + 2 * b_bits + b_fl, s));
  char* at = ws;
  auto take = [&](size_t b) { char* p = at; at += b; return p; };
  bgs::GcArgs a{};
  a.rate = (const float*)d_rate;
  a.excess = (int*)take(b_int), a.height = (int*)take(b_int), a.resid = (int*)take(b_int);
  a.ctl = (int*)take(b_ctl), a.negatives = a.ctl + 3 * (size_t)budget;
  a.labels = d_labels ? (uint8_t*)d_labels : (uint8_t*)take(b_lab);
  a.flow = (int*)d_flow, a.stats = stats;
  a.images = images, a.nh = nh, a.nw = nw, a.budget = budget, a.weight = min_cut_weight;
  uint8_t *nodes = (uint8_t*)take(b_px), *filled = (uint8_t*)take(b_px);
  uint64_t *mb = (uint64_t*)take(b_bits), *rb = (uint64_t*)take(b_bits);
  int* fl = (int*)take(b_fl);
  (void)hipMemsetAsync(a.ctl, 0, b_ctl, s);
  (void)hipMemsetAsync(fl, 0, b_fl, s);
  bgs::gc_solve_launch(a, s);
  bgs::lm_node_mask_launch(a.labels, nodes, images, rows, cols, histogram_area, nh, nw, s);
  // cvFloodFill from (0, 0): SuBSENSE's device flood fill (the seed value is the corner's own, always 0 here)
  hipLaunchKernelGGL(bgs::ss_flood_pack_kernel, dim3(blocks_for((size_t)rows * W64 * bgs::kWave), 1, images), dim3(bgs::kBlock), 0, s, (const uint8_t*)nodes, mb, rb, rows, cols, W64);
  hipLaunchKernelGGL(bgs::ss_flood_seed_kernel, dim3(images), dim3(bgs::kBlock), 0, s, (const uint64_t*)mb, rb, rows, cols, W64);
  const dim3 fgrid(blocks_for((size_t)tilesY * W64 * bgs::kWave), 1, images);
  for (int k = 0; k < bgs::kSsFloodBatch; ++k) ss_launch_flood(fgrid, images, tilesY, s, mb, rb, rows, W64, fl, k);
  hipLaunchKernelGGL(bgs::ss_flood_finish_kernel, dim3(images), dim3(256), 0, s, (const uint64_t*)mb, rb, rows, W64, fl, bgs::kSsFloodBatch);
  bgs::lm_paint_launch(rb, filled, images, rows, cols, W64, s);
  bgs::morph_launch(bgs::MorphArgs{filled, (uint8_t*)d_mask, rows, cols, 0, 3}, images, s);  // cvErode(…, NULL, 1)
  hipError_t er = hipGetLastError();
  hipError_t fr = hipFreeAsync(ws, s);
  if (er != hipSuccess || fr != hipSuccess) return fail(BGS_ERR_HIP, "bgs_lbpmrf_mask_device: %s", hipGetErrorString(er != hipSuccess ? er : fr));
  return BGS_OK;
}

// ---- the model stage of SJN_MultiCueBGS (engine_multicue.h)
int bgs_multicue_default_params(bgs_multicue_params* p) {
  if (!p) return fail(BGS_ERR_INVALID, "params is NULL");
  mc_defaults(p);
  return BGS_OK;
}

static const bgs_multicue_params* mc_arg(const bgs_multicue_params* p, bgs_multicue_params& d) {
  if (!p) return mc_defaults(&d), &d;
  if (p->struct_size != sizeof(*p)) return fail(BGS_ERR_INVALID, "bgs_multicue_params.struct_size %u != %zu (ABI mismatch)", p->struct_size, sizeof(*p)), nullptr;
  return p;
}

int bgs_multicue_check(const bgs_multicue_params* p, int rows, int cols) {
  bgs_multicue_params d;
  if (!(p = mc_arg(p, d))) return BGS_ERR_INVALID;
  int rc = mc_check((bgs_algo)0, *p);
  if (rc || rows == 0) return rc;
  if (rows < 0 || cols <= 0) return fail(BGS_ERR_INVALID, "bgs_multicue_check: bad geometry");
  return mc_check_geometry((bgs_algo)0, rows, cols, 3);
}

int bgs_multicue_create(int hip_device, int n_streams, const bgs_multicue_params* p, bgs_multicue** m) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_create: NULL argument");
  *m = nullptr;
  if (n_streams < 1 || n_streams > 65535) return fail(BGS_ERR_INVALID, "bgs_multicue_create: n_streams must be 1..65535");
  bgs_multicue_params d;
  if (!(p = mc_arg(p, d))) return BGS_ERR_INVALID;
  int rc = mc_check((bgs_algo)0, *p);
  if (rc) return rc;
  bgs_multicue* o = new (std::nothrow) bgs_multicue();
  if (!o) return fail(BGS_ERR_NOMEM, "out of memory");
  rc = mc_create(hip_device, n_streams, p, o);
  if (rc) {
    delete o;
    return rc;
  }
  *m = o;
  return BGS_OK;
}

void bgs_multicue_destroy(bgs_multicue* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();
  delete m;
}

int bgs_multicue_train_device(bgs_multicue* m, const void* d_frames, int rows, int cols, void* hip_stream) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_train_device: NULL argument");
  return mc_train(*m, d_frames, rows, cols, (hipStream_t)hip_stream);
}

int bgs_multicue_landmark_device(bgs_multicue* m, const void* d_frames, int rows, int cols, void* d_landmark, void* d_conf, void* hip_stream) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_landmark_device: NULL argument");
  return mc_landmark(*m, d_frames, rows, cols, d_landmark, d_conf, (hipStream_t)hip_stream);
}

int bgs_multicue_update_device(bgs_multicue* m, const void* d_update_map, int ghost, void* hip_stream) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_update_device: NULL argument");
  return mc_update(*m, d_update_map, ghost, (hipStream_t)hip_stream);
}

int bgs_multicue_boxes_device(bgs_multicue* m, const void* d_landmark, const void* d_frames, int rows, int cols, void* d_fore, void* d_ghost_map, void* d_update_map,
                              void* d_count, void* d_boxes, void* hip_stream) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_boxes_device: NULL argument");
  return mc_boxes(*m, d_landmark, d_frames, rows, cols, d_fore, d_ghost_map, d_update_map, d_count, d_boxes, (hipStream_t)hip_stream);
}

int bgs_multicue_process_device(bgs_multicue* m, const void* d_frames, int rows, int cols, void* d_out, void* hip_stream) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_process_device: NULL argument");
  return mc_process_range(*m, "bgs_multicue_process_device", 0, m->S, d_frames, rows, cols, d_out, (hipStream_t)hip_stream);
}

int bgs_multicue_process_range_device(bgs_multicue* m, int first, int count, const void* d_frames, int rows, int cols, void* d_out, void* hip_stream) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_process_range_device: NULL argument");
  return mc_process_range(*m, "bgs_multicue_process_range_device", first, count, d_frames, rows, cols, d_out, (hipStream_t)hip_stream);
}

int bgs_multicue_reset_stream(bgs_multicue* m, int stream) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_reset_stream: NULL argument");
  return mc_reset_stream(*m, stream);
}

int bgs_multicue_process(bgs_multicue* m, int stream, const void* frame, int rows, int cols, size_t step, void* out, size_t out_step, int out_channels) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_process: NULL argument");
  return mc_process_host(*m, stream, frame, rows, cols, step, out, out_step, out_channels);
}

int64_t bgs_multicue_get_state(bgs_multicue* m, int stream, const char* plane, void* dst, size_t cap) {
  if (!m) return fail(BGS_ERR_INVALID, "bgs_multicue_get_state: NULL argument");
  return mc_get_state(*m, stream, plane, dst, cap);
}

int bgs_multicue_xyz_device(int hip_device, const void* d_bgr, void* d_xyz, size_t pixels, void* hip_stream) {
  if (!d_bgr || !d_xyz || !pixels || pixels > ((size_t)1 << 31)) return fail(BGS_ERR_INVALID, "bgs_multicue_xyz_device: bad argument");
  HIP_TRY(hipSetDevice(hip_device));
  hipLaunchKernelGGL(bgs::mc_xyz_kernel, dim3(blocks_for(pixels)), dim3(bgs::kBlock), 0, (hipStream_t)hip_stream, (const uint8_t*)d_bgr, (uint8_t*)d_xyz, pixels);
  HIP_TRY(hipGetLastError());
  return BGS_OK;
}

size_t bgs_mask_components_workspace(int rows, int cols) { return bgs_mask_components_batch_workspace(1, rows, cols); }

size_t bgs_mask_components_batch_workspace(int images, int rows, int cols) {
  if (images <= 0 || rows <= 0 || cols <= 0) return 0;
  const size_t n = (size_t)images * rows * cols, nb = (n + bgs::kCcPerBlock - 1) / bgs::kCcPerBlock;
  return (2 * n + nb + 16) * sizeof(int32_t);  // labels (when the caller passes none) + ids + per-block root counts
}

// images stacked back to back are labelled as one tall image whose links never cross an image boundary
static int cc_run(int hip_device, const void* d_mask, int images, int rows, int cols, int connectivity, int32_t* d_labels, bgs_box* d_boxes, int max_boxes,
                  int32_t* d_count, int32_t* d_offsets, void* d_work, void* hip_stream, bgs_moments* d_moments = nullptr) {
  static_assert(sizeof(bgs_moments) == sizeof(bgs::CcMoments), "bgs_moments layout");
  static_assert(sizeof(bgs_box) == sizeof(bgs::CcBox), "bgs_box layout");
  if (!d_mask || !d_boxes || (!d_count && !d_offsets) || images <= 0 || rows <= 0 || cols <= 0 || max_boxes < 0 || (connectivity != 4 && connectivity != 8))
    return fail(BGS_ERR_INVALID, "bgs_mask_components: bad argument");
  const size_t imgN = (size_t)rows * cols, n = imgN * images;
  if (n >= (size_t)0x7fffffff) return fail(BGS_ERR_UNSUPPORTED, "bgs_mask_components: too many pixels for 32-bit labels");
  HIP_TRY(hipSetDevice(hip_device));
  hipStream_t s = (hipStream_t)hip_stream;
  void* own = nullptr;
  if (!d_work) {
    HIP_TRY(hipMalloc(&own, bgs_mask_components_batch_workspace(images, rows, cols)));
    d_work = own;
  }
  const int nb = (int)((n + bgs::kCcPerBlock - 1) / bgs::kCcPerBlock);
  int* id = (int*)d_work;
  int* L = d_labels ? (int*)d_labels : id + n;
  int* blockCount = id + 2 * n;
  int* total = d_count ? (int*)d_count : blockCount + nb;  // scratch slot when only offsets are wanted
  const int conn8 = connectivity == 8, allRows = rows * images;
  const dim3 grid(blocks_for(n)), block(bgs::kBlock);
  if (d_offsets) HIP_TRY(hipMemsetAsync(d_offsets, 0, ((size_t)images + 1) * sizeof(int32_t), s));
  if (d_moments && max_boxes > 0) HIP_TRY(hipMemsetAsync(d_moments, 0, (size_t)max_boxes * sizeof(bgs_moments), s));
  hipLaunchKernelGGL(bgs::cc_init_kernel, grid, block, 0, s, (const uint8_t*)d_mask, L, allRows, cols, rows, conn8);
  hipLaunchKernelGGL(bgs::cc_merge_kernel, grid, block, 0, s, L, allRows, cols, rows, conn8);
  hipLaunchKernelGGL(bgs::cc_compress_kernel, grid, block, 0, s, L, n);
  hipLaunchKernelGGL(bgs::cc_count_kernel, dim3(nb), block, 0, s, (const int*)L, n, blockCount);
  hipLaunchKernelGGL(bgs::cc_scan_kernel, dim3(1), block, 0, s, blockCount, nb, total);
  hipLaunchKernelGGL(bgs::cc_scatter_kernel, dim3(nb), block, 0, s, (const int*)L, n, (const int*)blockCount, id, (bgs::CcBox*)d_boxes, max_boxes, (int*)d_offsets, imgN);
  if (max_boxes > 0) {
    hipLaunchKernelGGL(bgs::cc_boxes_kernel, dim3(blocks_for((n + bgs::kCcBoxPer - 1) / bgs::kCcBoxPer)), block, 0, s, (const int*)L, (const int*)id, allRows, cols, rows, (bgs::CcBox*)d_boxes, max_boxes, (bgs::CcMoments*)d_moments);
    hipLaunchKernelGGL(bgs::cc_finish_kernel, dim3(blocks_for((size_t)max_boxes)), block, 0, s, (bgs::CcBox*)d_boxes, (const int*)total, max_boxes, (int)imgN);
  }
  if (d_offsets) hipLaunchKernelGGL(bgs::cc_offsets_kernel, dim3(1), dim3(1), 0, s, (int*)d_offsets, images);
  if (d_labels && images > 1) hipLaunchKernelGGL(bgs::cc_localize_kernel, grid, block, 0, s, L, n, imgN);
  hipError_t er = hipGetLastError();
  if (own) {
    const hipError_t e2 = hipStreamSynchronize(s);
    if (er == hipSuccess) er = e2;
    (void)hipFree(own);
  }
  if (er != hipSuccess) return fail(BGS_ERR_HIP, "connected components failed: %s", hipGetErrorString(er));
  return BGS_OK;
}

int bgs_mask_components_device(int hip_device, const void* d_mask, int rows, int cols, int connectivity, int32_t* d_labels, bgs_box* d_boxes, int max_boxes,
                               int32_t* d_count, void* d_work, void* hip_stream) {
  if (!d_count) return fail(BGS_ERR_INVALID, "bgs_mask_components_device: d_count is NULL");
  return cc_run(hip_device, d_mask, 1, rows, cols, connectivity, d_labels, d_boxes, max_boxes, d_count, nullptr, d_work, hip_stream);
}

int bgs_mask_components_batch_device(int hip_device, const void* d_masks, int images, int rows, int cols, int connectivity, int32_t* d_labels, bgs_box* d_boxes,
                                     int max_boxes, int32_t* d_offsets, void* d_work, void* hip_stream) {
  if (!d_offsets) return fail(BGS_ERR_INVALID, "bgs_mask_components_batch_device: d_offsets is NULL");
  return cc_run(hip_device, d_masks, images, rows, cols, connectivity, d_labels, d_boxes, max_boxes, nullptr, d_offsets, d_work, hip_stream);
}

int bgs_mask_blobs_batch_device(int hip_device, const void* d_masks, int images, int rows, int cols, int connectivity, bgs_box* d_boxes, bgs_moments* d_moments,
                                int max_boxes, int32_t* d_offsets, void* d_work, void* hip_stream) {
  if (!d_offsets) return fail(BGS_ERR_INVALID, "bgs_mask_blobs_batch_device: d_offsets is NULL");
  return cc_run(hip_device, d_masks, images, rows, cols, connectivity, nullptr, d_boxes, max_boxes, nullptr, d_offsets, d_work, hip_stream, d_moments);
}

int bgs_last_mask_blobs(bgs_engine* e, int stream, int connectivity, int min_w, int min_h, bgs_box* boxes, bgs_moments* moments, int max_boxes, int32_t* count) {
  if (!e || !count || max_boxes < 0 || (max_boxes > 0 && !boxes)) return fail(BGS_ERR_INVALID, "bgs_last_mask_blobs: bad argument");
  *count = 0;
  if (stream < 0 || stream >= e->S) return fail(BGS_ERR_INVALID, "stream %d outside 0..%d", stream, e->S - 1);
  if (!e->n || e->last_fg_stream != stream)
    return fail(BGS_ERR_STATE, "bgs_last_mask_blobs: the last bgs_process call left no valid mask of stream %d on the device", stream);
  HIP_TRY(hipSetDevice(e->device));
  // device scratch, grown on demand: [workspace][boxes cap][moments cap][count].  The component pass keeps the first `cap` components in
  // raster order and COUNTS all of them; the size filter below runs on the host, so every component has to be kept: when a mask
  // holds more than the scratch has room for (an unfiltered FrameDifference mask can carry thousands of one-pixel speckles before the
  // first real blob), the scratch is regrown to the true total and the pass repeated - otherwise late large blobs would be lost.
  const size_t ws = (bgs_mask_components_workspace(e->rows, e->cols) + 15) & ~(size_t)15;
  int cap = std::max(std::max(max_boxes, 1024), e->cc_cap);
  int32_t n = 0;
  bgs_box* d_boxes = nullptr;
  bgs_moments* d_mom = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    if (!e->cc_work || e->cc_cap < cap) {
      if (e->cc_work) (void)hipFree(e->cc_work), e->cc_work = nullptr, e->cc_cap = 0;
  if (e->pack_fg) (void)hipFree(e->pack_fg), e->pack_fg = nullptr, e->pack_fg_bytes = 0;
      HIP_TRY(hipMalloc(&e->cc_work, ws + (size_t)cap * (sizeof(bgs_box) + sizeof(bgs_moments)) + 16));
      e->cc_cap = cap;
    }
    d_boxes = (bgs_box*)((char*)e->cc_work + ws);
    d_mom = (bgs_moments*)(d_boxes + e->cc_cap);
    int32_t* d_count = (int32_t*)(d_mom + e->cc_cap);
    int rc = cc_run(e->device, e->host.sync.fg.d, 1, e->rows, e->cols, connectivity, nullptr, d_boxes, e->cc_cap, d_count, nullptr, e->cc_work, e->stream(), d_mom);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(&n, d_count, sizeof(n), hipMemcpyDeviceToHost, e->stream()));
    HIP_TRY(hipStreamSynchronize(e->stream()));
    if (n <= e->cc_cap) break;
    cap = n + n / 8 + 64;  // the true total is known now: one more pass with room for all of them
  }
  n = std::min(n, e->cc_cap);  // (cannot bind after the second pass: the mask has not changed)
  std::vector<bgs_box> hb((size_t)n);
  std::vector<bgs_moments> hm((size_t)n);
  if (n) {
    { const int rc__ = d2h_staged(hb.data(), d_boxes, (size_t)n * sizeof(bgs_box)); if (rc__ != BGS_OK) return rc__; }
    { const int rc__ = d2h_staged(hm.data(), d_mom, (size_t)n * sizeof(bgs_moments)); if (rc__ != BGS_OK) return rc__; }
  }
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    if (hb[i].w < min_w || hb[i].h < min_h) continue;
    if (kept < max_boxes) {
      boxes[kept] = hb[i];
      if (moments) moments[kept] = hm[i];
    }
    ++kept;
  }
  *count = kept;
  return BGS_OK;
}

// ------------------------------------------------------------------------------------------------------------- N3: ingest

int bgs_set_ingest(bgs_engine* e, const bgs_ingest* c) {
  if (!e) return fail(BGS_ERR_INVALID, "engine is NULL");
  if (e->n) return fail(BGS_ERR_INVALID, "bgs_set_ingest must come before the first frame (it decides the engine's geometry)");
  if (!c) {
    e->ingest_on = false;
    return BGS_OK;
  }
  if (c->struct_size != sizeof(bgs_ingest)) return fail(BGS_ERR_INVALID, "bgs_ingest.struct_size mismatch");
  if (c->resize_percent <= 0) return fail(BGS_ERR_INVALID, "resize_percent must be positive");
  e->ingest = *c, e->ingest_on = true;
  return BGS_OK;
}

int bgs_ingest_default(bgs_ingest* c) {
  if (!c) return fail(BGS_ERR_INVALID, "cfg is NULL");
  std::memset(c, 0, sizeof(*c));
  c->struct_size = (uint32_t)sizeof(*c);
  c->resize_percent = 100;  // config/VideoCapture.xml, config/PreProcessor.xml: everything else off
  return BGS_OK;
}

int bgs_ingest_size(const bgs_ingest* c, int src_rows, int src_cols, int* rows, int* cols) {
  IngestPlan pl;
  int rc = ingest_plan(c, src_rows, src_cols, &pl);
  if (rc) return rc;
  if (rows) *rows = pl.rows;
  if (cols) *cols = pl.cols;
  return BGS_OK;
}

size_t bgs_ingest_workspace(const bgs_ingest* c, int images, int src_rows, int src_cols, int channels) {
  IngestPlan pl;
  if (images <= 0 || ingest_plan(c, src_rows, src_cols, &pl)) return 0;
  size_t need = 0;
  if (c->equalize_hist) need += (size_t)images * 256 * (sizeof(unsigned) + 1);
  if (c->gaussian_blur) need += (size_t)images * pl.rows * pl.cols * channels;  // the frame before the blur
  return need ? need + 64 : 0;
}

int bgs_ingest_device(int hip_device, const bgs_ingest* c, const void* d_src, int images, int src_rows, int src_cols, int channels, size_t src_step, void* d_dst,
                      void* d_work, void* hip_stream) {
  IngestPlan pl;
  int rc = ingest_plan(c, src_rows, src_cols, &pl);
  if (rc) return rc;
  if (!d_src || !d_dst || images <= 0 || images > 65535) return fail(BGS_ERR_INVALID, "bgs_ingest_device: bad argument");
  if (channels != 1 && channels != 3) return fail(BGS_ERR_UNSUPPORTED, "channels must be 1 or 3");
  if (src_step < (size_t)src_cols * channels) return fail(BGS_ERR_INVALID, "src_step %zu < src_cols*channels", src_step);
  if (c->equalize_hist && channels != 1) return fail(BGS_ERR_UNSUPPORTED, "equalizeHist needs a 1-channel frame (cv::equalizeHist asserts CV_8UC1, PreProcessor.cpp:64)");
  const size_t ws = bgs_ingest_workspace(c, images, src_rows, src_cols, channels);
  if (ws && !d_work) return fail(BGS_ERR_INVALID, "bgs_ingest_device: this configuration needs %zu bytes of d_work", ws);
  HIP_TRY(hipSetDevice(hip_device));
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t n = (size_t)pl.rows * pl.cols;
  // workspace: [hist][lut][pad to 16][pre-blur frames]
  unsigned* hist = (unsigned*)d_work;
  uint8_t* lut = (uint8_t*)d_work + (c->equalize_hist ? (size_t)images * 256 * sizeof(unsigned) : 0);
  uint8_t* pre = (uint8_t*)(((uintptr_t)(lut + (c->equalize_hist ? (size_t)images * 256 : 0)) + 15) & ~(uintptr_t)15);
  uint8_t* geom_out = c->gaussian_blur ? pre : (uint8_t*)d_dst;
  bgs::IngestArgs a{};
  a.src = (const uint8_t*)d_src, a.dst = geom_out, a.src_rows = src_rows, a.src_cols = src_cols, a.rw = pl.rw, a.rh = pl.rh, a.rows = pl.rows, a.cols = pl.cols;
  a.x0 = pl.x0, a.y0 = pl.y0, a.flip = c->flip != 0, a.mode = pl.mode, a.src_step = src_step, a.scale_x = pl.scale_x, a.scale_y = pl.scale_y;
  const dim3 grid(blocks_for(n), 1, images), block(bgs::kBlock);
  if (channels == 3)
    hipLaunchKernelGGL((bgs::ingest_geom_kernel<3>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((bgs::ingest_geom_kernel<1>), grid, block, 0, s, a);
  if (c->equalize_hist) {
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)images * 256 * sizeof(unsigned), s));
    hipLaunchKernelGGL(bgs::ingest_hist_kernel, dim3(std::min<unsigned>(blocks_for(n), 1024), 1, images), block, 0, s, (const uint8_t*)geom_out, n, hist);
    hipLaunchKernelGGL(bgs::ingest_lut_kernel, dim3(images), block, 0, s, (const unsigned*)hist, lut, (unsigned)n);
    hipLaunchKernelGGL(bgs::ingest_apply_lut_kernel, grid, block, 0, s, geom_out, n, (const uint8_t*)lut);
  }
  if (c->gaussian_blur) {
    bgs::BlurArgs b{};
    b.src = pre, b.dst = (uint8_t*)d_dst, b.rows = pl.rows, b.cols = pl.cols;
    gaussian7_kernel(b.k);
    const dim3 bgrid((pl.cols + bgs::kBlurTW - 1) / bgs::kBlurTW, (pl.rows + bgs::kBlurTH - 1) / bgs::kBlurTH, images);
    if (channels == 3)
      hipLaunchKernelGGL((bgs::ingest_blur7_kernel<3>), bgrid, block, 0, s, b);
    else
      hipLaunchKernelGGL((bgs::ingest_blur7_kernel<1>), bgrid, block, 0, s, b);
  }
  HIP_TRY(hipGetLastError());
  return BGS_OK;
}

int bgs_ingest_host(int hip_device, const bgs_ingest* c, const uint8_t* src, int src_rows, int src_cols, int channels, size_t src_step, uint8_t* dst, size_t dst_step) {
  IngestPlan pl;
  int rc = ingest_plan(c, src_rows, src_cols, &pl);
  if (rc) return rc;
  if (!src || !dst) return fail(BGS_ERR_INVALID, "bgs_ingest_host: NULL buffer");
  if (channels != 1 && channels != 3) return fail(BGS_ERR_UNSUPPORTED, "channels must be 1 or 3");
  const size_t out_row = (size_t)pl.cols * channels;
  if (dst_step < out_row) return fail(BGS_ERR_INVALID, "dst_step %zu < cols*channels", dst_step);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(BGS_ERR_HIP, "no HIP device visible: libbgs_hip has no CPU path");
  HIP_TRY(hipSetDevice(hip_device));
  const size_t in_bytes = (size_t)src_rows * src_cols * channels, out_bytes = (size_t)pl.rows * out_row, ws = bgs_ingest_workspace(c, 1, src_rows, src_cols, channels);
  const size_t in_row = (size_t)src_cols * channels;
  Staging work;  // bgs_ingest_device's workspace; outlives the lane, whose destructor drains the stream
  Lane ln;       // of this call alone: the raw frame as `in`, the prepared one as `fg`; released on every way out
  hipError_t er = ln.make(in_bytes, out_bytes, 0);
  if (er == hipSuccess) er = work.make(ws, /*host=*/false);
  if (er == hipSuccess) er = upload_rows(ln.in, ln.in.d, ln.hs, src, src_step, in_row, src_rows, 1);
  if (er != hipSuccess) return (void)hipGetLastError(), fail(BGS_ERR_HIP, "bgs_ingest_host: %s", hipGetErrorString(er));
  rc = bgs_ingest_device(hip_device, c, ln.in.d, 1, src_rows, src_cols, channels, in_row, ln.fg.d, work.d, ln.hs);
  if (rc) return rc;  // ~Lane drains the stream
  er = download_whole(ln.fg, out_bytes, ln.hs);
  if (er == hipSuccess) er = hipStreamSynchronize(ln.hs);
  if (er != hipSuccess) return fail(BGS_ERR_HIP, "bgs_ingest_host: %s", hipGetErrorString(er));
  unpack_rows(dst, dst_step, ln.fg.h, out_row, 0, pl.rows);
  return BGS_OK;
}


}  // extern "C"

namespace {
void mc_launch_resize(const bgs::IngestArgs& g, unsigned streams, hipStream_t s) {  // engine_multicue.h
  hipLaunchKernelGGL((bgs::ingest_geom_kernel<1>), dim3(blocks_for((size_t)g.rows * g.cols), 1, streams), dim3(bgs::kBlock), 0, s, g);
}
}  // namespace

#include "engine_group.h"
