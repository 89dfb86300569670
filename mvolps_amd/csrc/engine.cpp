// engine.cpp -- host side of the MI355X dense-simplex engine: device context, per-handle
// HBM slabs, the queued pivot loop, tableau maintenance under model edits, and the export
// of basis / solution mirrors.  Counterpart of glp_simplex and the glp_* edit calls MVOLPS
// makes (/root/reference/bs.cpp:114-117,274-288; cut.cpp:23-43).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <functional>
#include <limits>
#include <map>
#include <mutex>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "engine.hpp"

// Device copy of model rows 1..m0 (see mvx_prob::dmat).  `plain` is indexed by column; `packed` holds each row's
// non-zeros side by side (what position k of glp_get_mat_row's list means, gmi.cpp:84-87) and is the same buffer
// when every row is dense.
struct DevMatrix {
  int m0 = 0, n = 0, lda = 0;
  double *plain = nullptr, *packed = nullptr;
  int *len = nullptr; // nullptr: every row has n non-zeros
  std::vector<mvx::RowPtr> rows; // the host rows this was built from, owned: a row's address cannot be reused while compared against
  ~DevMatrix() {
    if (packed && packed != plain) (void)hipFree(packed);
    if (plain) (void)hipFree(plain);
    if (len) (void)hipFree(len);
  }
};

// Device copy of a root's model for the rounding heuristic (see mvx_prob::rmod, engine_round_many), and the host state it
// was built from: it is rebuilt when any of that has changed.
struct RoundModel {
  int m0 = 0, n = 0, ldm = 0, dir = 0;
  void *dev = nullptr; // [At (n+1) x ldm][rlo m0][rhi m0][clo n+1][chi n+1][c n+1][flags n+1][dl n+1][ul n+1][len n+1]
  void *dev_rows = nullptr; // [Ar m0 x ldn]: the same rows by row, for k_prop; uploaded on the first propagation
  int ldn = 0;
  void *dev_graph = nullptr; // [adj (n+1) x W][member n+1]: the conflict graph for k_cliquesep, computed on its first call
  size_t o_member = 0;
  size_t o_rlo = 0, o_rhi = 0, o_clo = 0, o_chi = 0, o_c = 0, o_flags = 0;
  size_t o_dl = 0, o_ul = 0, o_len = 0; // per column: rows that lock it down / up, its non-zeros (k_divepick)
  std::vector<mvx::RowPtr> rows; // owned: a row's address cannot be reused while the model compares against it
  std::vector<double> c, clb, cub, rlb, rub;
  std::vector<int> kind;
  ~RoundModel() {
    if (dev) (void)hipFree(dev);
    if (dev_rows) (void)hipFree(dev_rows);
    if (dev_graph) (void)hipFree(dev_graph);
  }
};

namespace mvx {

#define HIPCHECK(expr)                                                                         \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      std::fprintf(stderr, "mvx: HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, __LINE__, #expr); \
      std::abort();                                                                            \
    }                                                                                          \
  } while (0)

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// lays pieces out one after the other on 256-byte boundaries: carve(bytes) is the piece's offset, `off` the total so far
struct Carver {
  size_t off = 0;
  size_t operator()(size_t bytes) {
    size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  }
};

// Names a buffer's pieces once for both passes over them: piece(p, count) carves count elements of p's type and, given
// the allocation's base, points p at them; with a null base the walk only measures (carve.off is the total).
struct Pieces {
  unsigned char *base;
  Carver carve;
  template <class T>
  void operator()(T *&p, size_t count) {
    const size_t o = carve(count * sizeof(T));
    if (base) p = (T *)(base + o);
  }
};

// ------------------------------------------------------------------------------ context
// One solve context = one HIP stream with its own control block, scratch and staging.  The main
// context serves every single-handle call; mvx_simplex_batch has its own (BatchCtx below).
constexpr size_t XG_BYTES = 4 * 8 * 64 * 16; // k_chain's exchange area: 4 regions x 8 fields x 64 records x 16 bytes
struct SolveCtx {
  hipStream_t stream = nullptr;
  Ctl *d_ctl = nullptr;
  Ctl *h_ctl = nullptr; // pinned
  // scratch sized for the largest problem seen
  int sc_m_cap = 0, sc_ld = 0;
  void *scratch = nullptr;
  double *d_colq = nullptr, *d_srow = nullptr, *d_cost1 = nullptr, *d_wts = nullptr, *d_part = nullptr, *d_rcbase = nullptr;
  int *d_gflag = nullptr;
  double *d_colqx[2] = {nullptr, nullptr}, *d_betac[2] = {nullptr, nullptr};
  double *d_dw = nullptr, *d_dw2 = nullptr; // dual devex weights by row, two sets (fused dual path ping-pong)
  int *d_p1list = nullptr; // phase 1: rows whose infeasibility sign changed
  int *d_tflag = nullptr;  // tableau refresh: target non-basic status by variable number
  double *d_pw[2] = {nullptr, nullptr}; // primal devex weights by column, two sets (fused path ping-pong)
  double *d_srowk[KCH] = {}, *d_colqk[KCH] = {}; // chained primal path: scaled pivot rows / pivot columns of the steps
  // chained primal path: what a step changes besides the tableau, in two alternating sets (ChainArgs), and the partials
  double *d_drowk[2] = {}, *d_pwk[2] = {}, *d_nlbk[2] = {}, *d_nubk[2] = {}, *d_betak[2] = {}, *d_blbk[2] = {}, *d_bubk[2] = {};
  int *d_nflagk[2] = {};
  double *d_betab = nullptr, *d_ppart = nullptr, *d_rpart = nullptr;
  double *d_zeros = nullptr; // chained primal path: zeros (bound-flip operands of the bulk pass)
  // row combinations queued without a host round trip each (cut rows of a B&B round): a ring of pinned staging slots
  // (control block, row weights, base row); the stream is synchronised only when the ring wraps
  unsigned char *rc_ring = nullptr;
  size_t rc_slot_bytes = 0;
  int rc_next = 0, rc_m_cap = 0, rc_ld = 0;
  // cluster selection (k_chain): exchange area, abort flag, tag of the next launch's first exchange
  unsigned *d_xg = nullptr;
  int *d_xabort = nullptr;
  unsigned xtag = 0;
  size_t pp_stride = 0, rp_stride = 0;
  size_t sk_stride = 0, ck_stride = 0; // doubles between the chain's consecutive scaled pivot rows / pivot columns
  Cand *d_rpc = nullptr;
  double *d_olb = nullptr, *d_oub = nullptr; // bounds by variable number, saved by the anti-stalling perturbation
  Cand *d_pp[2] = {nullptr, nullptr}, *d_rp = nullptr;
  // staging area of k_export.  Default: ONE pinned host buffer that the kernel writes straight over PCIe (d_stage is its
  // device-side address): no device-to-host copy behind the last kernel of a call (~16 us: 12 us to start the copy
  // engine, 4 us of copy).  MVX_ZC_STAGE=0: a device buffer and a copy, as before.
  unsigned char *d_stage = nullptr, *h_stage = nullptr;
  bool stage_zc = false;
  size_t stage_bytes = 0;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  // resident-tableau path (k_persist): candidate granules, pivot messages, abort flag; a backup of the slab, the
  // control block and the devex weights taken in front of every launch, put back if the launch aborts
  unsigned long long *d_pcand = nullptr, *d_pmsg = nullptr;
  int *d_pabort = nullptr, *h_pabort = nullptr;
  int p_msg_words = 0;
  void *p_backup = nullptr;
  size_t p_backup_bytes = 0;
  Ctl *d_pctl = nullptr;
  double *d_ppw = nullptr;
  int p_pw_ld = 0;
};

// Slabs carved out of one multi-slab allocation (a growing B&B tree asks for one slab per open node: hipMalloc
// costs ~60 us a call, a chunk of up to 32 amortises it).  An arena goes back to the driver only whole, when every
// slab of it is idle.
struct Arena {
  void *base = nullptr;
  size_t slab_bytes = 0;
  int count = 0, idle = 0;
};

// Slab recycling (B&B clones come and go at one size).  Shared by the calling thread and the B&B driver's worker
// thread (bnb.cpp: child solves run on a worker while the caller clones and deletes other handles), hence the lock.
struct SlabCache {
  std::mutex mu;
  std::multimap<size_t, void *> free_slabs;
  std::unordered_map<void *, int> arena_of; // slab -> index into arenas
  std::vector<Arena> arenas;
  size_t idle_bytes = 0; // bytes held by idle slabs, arena slabs included
};

// The one device buffer + pinned host buffer of the batched node entries -- GMI cuts, classification, penalties, rounding,
// the diving pick, rc-tightening, propagation and the two bound-list entries (tighten, set bounds), all through NodeCall:
// descriptors go up through `host`, results come back into it -- written there by the kernel itself through `host_dev`, the
// pinned buffer's device address (null when it has none), or by a copy out of `dev`.
// Sharing rule: the pointers are valid from NodeCall::reserve until the entry's closing stream synchronise, under
// main_mu; an entry that holds pointers into it calls no other entry.
struct NodeScratch {
  void *dev = nullptr, *host = nullptr;
  unsigned char *host_dev = nullptr;
  size_t dev_bytes = 0, host_bytes = 0;
};

struct Context {
  int dev = -1;
  bool aux_ready = false;
  // every entry point that works on the main context (its stream, control block, scratch, staging buffer) holds
  // this lock: single-handle solves, model edits, clones, queries that refresh the mirrors
  std::recursive_mutex main_mu;
  SolveCtx main;
  // single-handle solves issued from inside a batch call (a lone pending handle, the phase-1 fallback) run on a
  // context of their own: the batch call may come from the B&B driver's worker thread while the calling thread
  // uses `main` for cut rows and solution queries
  SolveCtx aux;
  std::mutex aux_mu; // one single-handle solve at a time on `aux` (two batch calls may run on two threads)
  SlabCache slabs;
  // clones recorded by engine_copy and not yet launched (main_mu held): a round of B&B branchings makes one clone per
  // branching with only host-side work in between, so they leave as ONE k_copy_many launch when the next entry point
  // that touches device data arrives (flush_copies)
  std::vector<CopyJob> copies;
  NodeScratch nodes;
  // profiling (main context only)
  bool prof = false;
  double prof_update_ms = 0.0;
  long long prof_update_n = 0;
  std::vector<hipEvent_t> ev_pool;
};
#define MAIN_LOCK(c) std::lock_guard<std::recursive_mutex> main_lock_((c).main_mu)

static Context *g_ctx = nullptr;
static std::mutex g_ctx_mu;
static std::atomic<int> g_last_error{0}; // MVX_ENOMEM ...: read and cleared by mvx_last_error()
static int g_stall_limit = 0;      // > 0: overrides 64 + (m+n)/8 (tests drive the anti-stalling rules with it)
static int g_requested_dev = -1;

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int set_device(int dev) {
  if (g_ctx && g_ctx->dev != dev) return -1; // one device per process
  g_requested_dev = dev;
  return 0;
}

static void init_solve_ctx(SolveCtx &sc) {
  HIPCHECK(hipStreamCreateWithFlags(&sc.stream, hipStreamNonBlocking));
  HIPCHECK(hipMalloc((void **)&sc.d_ctl, sizeof(Ctl)));
  HIPCHECK(hipHostMalloc((void **)&sc.h_ctl, sizeof(Ctl)));
  HIPCHECK(hipEventCreate(&sc.ev_a));
  HIPCHECK(hipEventCreate(&sc.ev_b));
  HIPCHECK(hipMalloc((void **)&sc.d_xg, XG_BYTES + 256));
  HIPCHECK(hipMemsetAsync(sc.d_xg, 0, XG_BYTES + 256, sc.stream)); // ordered with the launches that use it (a null-stream memset is not)
  sc.d_xabort = (int *)((unsigned char *)sc.d_xg + XG_BYTES);
}

int take_last_error() { return g_last_error.exchange(0); }

// the current device is per host thread: a thread other than the one that made the first engine call binds itself
int bind_thread() {
  if (!g_ctx) return -1;
  return hipSetDevice(g_ctx->dev) == hipSuccess ? 0 : -1;
}

static Context &ctx() {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  if (g_ctx) return *g_ctx;
  int n = device_count();
  if (n <= 0) {
    std::fprintf(stderr,
                 "mvx: no HIP device visible -- the MI355X (gfx950) engine cannot run and this library has no CPU "
                 "fallback\n");
    std::abort();
  }
  Context *c = new Context();
  c->dev = g_requested_dev >= 0 ? g_requested_dev : 0;
  HIPCHECK(hipSetDevice(c->dev));
  init_solve_ctx(c->main);
  g_ctx = c;
  return *c;
}

// Binds the context's device for the calling thread, once per thread: clones, node entries and solution queries come
// from the B&B driver's helper threads too.
static void bind_device(const Context &c) {
  static thread_local bool bound = false;
  if (bound) return;
  HIPCHECK(hipSetDevice(c.dev));
  bound = true;
}

// Caller holds main_mu.  Grows c.nodes (see NodeScratch for the sharing rule) to at least dev_bytes / host_bytes, each
// side on its own and to 1.5 x the request; a call that fits costs two comparisons and does not touch the stream.
// false: out of memory -- the arena is left empty, mvx_last_error() reads MVX_ENOMEM, the entry returns -2.
static bool node_scratch_reserve(Context &c, size_t dev_bytes, size_t host_bytes) {
  NodeScratch &s = c.nodes;
  if (dev_bytes <= s.dev_bytes && host_bytes <= s.host_bytes) return true;
  HIPCHECK(hipStreamSynchronize(c.main.stream));
  bool ok = true;
  if (dev_bytes > s.dev_bytes) {
    if (s.dev) HIPCHECK(hipFree(s.dev));
    s.dev_bytes = dev_bytes + dev_bytes / 2;
    ok = hipMalloc(&s.dev, s.dev_bytes) == hipSuccess;
    if (!ok) s.dev = nullptr;
  }
  if (ok && host_bytes > s.host_bytes) {
    if (s.host) HIPCHECK(hipHostFree(s.host));
    s.host_dev = nullptr;
    s.host_bytes = host_bytes + host_bytes / 2;
    ok = hipHostMalloc(&s.host, s.host_bytes) == hipSuccess;
    void *dp = nullptr;
    if (!ok) s.host = nullptr;
    else if (hipHostGetDevicePointer(&dp, s.host, 0) == hipSuccess && dp) s.host_dev = (unsigned char *)dp;
    else (void)hipGetLastError();
  }
  if (ok) return true;
  (void)hipGetLastError();
  if (s.dev) HIPCHECK(hipFree(s.dev));
  if (s.host) HIPCHECK(hipHostFree(s.host));
  s = NodeScratch();
  g_last_error.store(MVX_ENOMEM);
  return false;
}

static void sync_batch_stream();
static void flush_copies(Context &c);
void sync_stream() {
  if (!g_ctx) return;
  {
    MAIN_LOCK(*g_ctx);
    flush_copies(*g_ctx);
  }
  HIPCHECK(hipStreamSynchronize(g_ctx->main.stream));
  sync_batch_stream();
}

// caller holds main_mu.  Launch the recorded clones on the main stream, COPY_BATCH ranges per launch.
static void flush_copies(Context &c) {
  if (c.copies.empty()) return;
  for (size_t k0 = 0; k0 < c.copies.size(); k0 += COPY_BATCH) {
    CopyBatch b;
    b.count = (int)std::min<size_t>(COPY_BATCH, c.copies.size() - k0);
    for (int k = 0; k < b.count; k++) b.jobs[k] = c.copies[k0 + (size_t)k];
    launch_copy_many(b, c.main.stream);
  }
  c.copies.clear();
}

// The call frame of a batched node entry: the main lock, the layout of the arena (pieces that go up, then results, then
// device-only scratch, in that order), the reservation, the one upload, where the kernel writes its results, and the closing
// copy back + synchronise.  What differs between the entries is said in the constructor's arguments, nowhere else.
enum class NodeFlush {
  AtEntry,      // the recorded clones leave first: a clone INTO one of the slabs the entry reads must have landed
  BeforeUpload, // the bound-list entries: only once there is device work, in front of its upload
  Never         // propagation: it reads the handles' host bounds only, and its handles are freshly cloned, unsolved
                // children -- flushing here would split the round's clones over more k_copy_many launches
};
enum class NodeResults {
  Pinned, // the kernel writes into the pinned buffer itself when it has a device address: no copy back
  Device, // the kernel writes device memory, fetch() copies back
  None    // nothing comes back: fetch() only synchronises (the pinned side is free for the next call)
};
class NodeCall {
  std::unique_lock<std::recursive_mutex> lock_;
  Carver carve_;
  size_t up_end_ = 0, out_end_ = 0;
  const NodeFlush flush_;
  const NodeResults where_;

public:
  Context *c = nullptr;
  unsigned char *hb = nullptr, *db = nullptr, *ob = nullptr; // pinned side, device side, where the results are written
  // device = false: the call has no device work (bound lists of handles without a tableau): no context, no lock
  NodeCall(NodeFlush flush, NodeResults where, bool device = true) : flush_(flush), where_(where) {
    if (!device) return;
    c = &ctx();
    bind_device(*c);
    lock_ = std::unique_lock<std::recursive_mutex>(c->main_mu);
    if (flush_ == NodeFlush::AtEntry) flush_copies(*c);
  }
  hipStream_t stream() const { return c->main.stream; }
  size_t up(size_t bytes) { // a piece of the upload
    const size_t o = carve_(bytes);
    up_end_ = out_end_ = carve_.off;
    return o;
  }
  size_t out(size_t bytes) { // a piece of the results: needs room on the pinned side too
    const size_t o = carve_(bytes);
    out_end_ = carve_.off;
    return o;
  }
  size_t dev(size_t bytes) { return carve_(bytes); } // device-only scratch
  // false: out of memory, the entry returns -2 (node_scratch_reserve)
  bool reserve() {
    if (!node_scratch_reserve(*c, carve_.off, out_end_)) return false;
    hb = (unsigned char *)c->nodes.host;
    db = (unsigned char *)c->nodes.dev;
    ob = where_ == NodeResults::Pinned && c->nodes.host_dev ? c->nodes.host_dev : db;
    return true;
  }
  void upload() {
    if (flush_ == NodeFlush::BeforeUpload) flush_copies(*c);
    HIPCHECK(hipMemcpyAsync(db, hb, up_end_, hipMemcpyHostToDevice, stream()));
  }
  // queues the copy back of the results in front of offset `end` (default: all of them) when the kernel wrote device memory
  void copy_back(size_t end = 0) {
    if (where_ != NodeResults::None && ob == db)
      HIPCHECK(hipMemcpyAsync(hb + up_end_, db + up_end_, (end ? end : out_end_) - up_end_, hipMemcpyDeviceToHost, stream()));
  }
  void sync() { HIPCHECK(hipStreamSynchronize(stream())); }
  void fetch() { // the results are on the pinned side when this returns
    copy_back();
    sync();
  }
};

// the common part of a node-entry descriptor
static NodeRef node_ref(const mvx_prob *P) { return NodeRef{P->d_T, P->d_bvar, P->d_nvar, P->d_nflag, P->d_nlb, P->d_nub, P->m, P->ld}; }

// every piece of a solve context's scratch, in layout order (see Pieces), and the strides of the two partial arrays, which
// size their pieces; returns the bytes of the whole
static size_t scratch_pieces(SolveCtx &sc, int mc, int l, unsigned char *base) {
  const size_t row = (size_t)mc + 1, col = (size_t)l, var = (size_t)mc + l + 1; // per tableau row / column / variable number
  const int nchunks = (mc + ROWCOMB_CHUNK - 1) / ROWCOMB_CHUNK + 1;
  Pieces piece{base};
  piece(sc.d_colq, row), piece(sc.d_srow, col), piece(sc.d_cost1, col);
  piece(sc.d_wts, row), piece(sc.d_rcbase, col), piece(sc.d_gflag, row);
  piece(sc.d_part, (size_t)nchunks * l);
  piece(sc.d_colqx[0], row), piece(sc.d_colqx[1], row);
  piece(sc.d_betac[0], row), piece(sc.d_betac[1], row);
  piece(sc.d_pp[0], (size_t)fused_npb(l)), piece(sc.d_pp[1], (size_t)fused_npb(l));
  piece(sc.d_rp, (size_t)fused_nrb_max(mc));
  piece(sc.d_olb, var), piece(sc.d_oub, var);
  piece(sc.d_dw, row), piece(sc.d_dw2, row);
  piece(sc.d_p1list, row + 1);
  piece(sc.d_pw[0], col), piece(sc.d_pw[1], col);
  piece(sc.d_tflag, var);
  piece(sc.d_rpc, (size_t)(mc + 255) / 256 + 1);
  for (int k = 0; k < KCH; k++) piece(sc.d_srowk[k], col);
  for (int k = 0; k < KCH; k++) piece(sc.d_colqk[k], row);
  for (int k = 0; k < 2; k++) {
    piece(sc.d_drowk[k], col), piece(sc.d_pwk[k], col), piece(sc.d_nlbk[k], col), piece(sc.d_nubk[k], col);
    piece(sc.d_nflagk[k], 2 * col); // as wide as its neighbours of doubles
    piece(sc.d_betak[k], row), piece(sc.d_blbk[k], row), piece(sc.d_bubk[k], row);
  }
  sc.pp_stride = align_up((size_t)chain_ncb(l) + 1, 32);
  sc.rp_stride = align_up((size_t)chain_nrb(mc) + 1, 32);
  piece(sc.d_betab, row), piece(sc.d_ppart, 8 * sc.pp_stride), piece(sc.d_rpart, 4 * sc.rp_stride);
  piece(sc.d_zeros, std::max(col, row) + 32);
  return piece.carve.off;
}

static void ensure_scratch(SolveCtx &sc, int m_cap, int ld) {
  if (m_cap <= sc.sc_m_cap && ld <= sc.sc_ld) return;
  HIPCHECK(hipStreamSynchronize(sc.stream));
  int mc = m_cap > sc.sc_m_cap ? m_cap : sc.sc_m_cap;
  int l = ld > sc.sc_ld ? ld : sc.sc_ld;
  if (sc.scratch) HIPCHECK(hipFree(sc.scratch));
  if (sc.d_stage && !sc.stage_zc) HIPCHECK(hipFree(sc.d_stage));
  if (sc.h_stage) HIPCHECK(hipHostFree(sc.h_stage));
  sc.d_stage = nullptr;
  const size_t bytes = scratch_pieces(sc, mc, l, nullptr);
  HIPCHECK(hipMalloc(&sc.scratch, bytes));
  HIPCHECK(hipMemsetAsync(sc.scratch, 0, bytes, sc.stream));
  scratch_pieces(sc, mc, l, (unsigned char *)sc.scratch);
  sc.sk_stride = (size_t)(sc.d_srowk[1] - sc.d_srowk[0]);
  sc.ck_stride = (size_t)(sc.d_colqk[1] - sc.d_colqk[0]);
  sc.stage_bytes = StageView::bytes(mc, l);
  HIPCHECK(hipHostMalloc((void **)&sc.h_stage, sc.stage_bytes));
  {
    static int zc = -1;
    if (zc < 0) {
      const char *e = std::getenv("MVX_ZC_STAGE");
      zc = e ? (std::atoi(e) != 0) : 1;
    }
    void *dp = nullptr;
    sc.stage_zc = zc && hipHostGetDevicePointer(&dp, sc.h_stage, 0) == hipSuccess && dp;
    if (sc.stage_zc) sc.d_stage = (unsigned char *)dp;
    else {
      (void)hipGetLastError();
      HIPCHECK(hipMalloc((void **)&sc.d_stage, sc.stage_bytes));
    }
  }
  sc.sc_m_cap = mc;
  sc.sc_ld = l;
}

// ------------------------------------------------------------------------------- slabs
struct SlabLayout {
  size_t o_T, o_bvar, o_blb, o_bub, o_nvar, o_nflag, o_nlb, o_nub, total;
};
static SlabLayout slab_layout(int m_cap, int ld) {
  SlabLayout L;
  Carver carve;
  L.o_T =carve((size_t)(m_cap + 1) * ld * 8);
  L.o_bvar = carve((size_t)(m_cap + 1) * 4);
  L.o_blb = carve((size_t)(m_cap + 1) * 8);
  L.o_bub = carve((size_t)(m_cap + 1) * 8);
  L.o_nvar = carve((size_t)ld * 4);
  L.o_nflag = carve((size_t)ld * 4);
  L.o_nlb = carve((size_t)ld * 8);
  L.o_nub = carve((size_t)ld * 8);
  L.total = carve.off;
  return L;
}

// the view of a raw slab laid out as L with row stride ld, and of the slab a handle is bound to
static SlabView slab_view_at(void *slab, const SlabLayout &L, int ld) {
  unsigned char *b = (unsigned char *)slab;
  return SlabView{(double *)(b + L.o_T),  (int *)(b + L.o_bvar),  (double *)(b + L.o_blb), (double *)(b + L.o_bub),
                  (int *)(b + L.o_nvar), (int *)(b + L.o_nflag), (double *)(b + L.o_nlb), (double *)(b + L.o_nub), ld};
}
static SlabView slab_view(const mvx_prob *P) {
  return SlabView{P->d_T, P->d_bvar, P->d_blb, P->d_bub, P->d_nvar, P->d_nflag, P->d_nlb, P->d_nub, P->ld};
}

static void bind_slab(mvx_prob *P, void *slab, int m_cap, int ld) {
  const SlabLayout L = slab_layout(m_cap, ld);
  const SlabView v = slab_view_at(slab, L, ld);
  P->slab = slab;
  P->slab_bytes = L.total;
  P->m_cap = m_cap;
  P->ld = ld;
  P->d_T = v.T;
  P->d_bvar = v.bvar, P->d_blb = v.blb, P->d_bub = v.bub;
  P->d_nvar = v.nvar, P->d_nflag = v.nflag, P->d_nlb = v.nlb, P->d_nub = v.nub;
  // debugging aid: MVX_BIND_FILL="t,a" fills the tableau region with byte t and the small arrays with byte a at every
  // binding (-1: leave), on the main stream (the caller's upload or clone follows on it)
  static const char *bf = std::getenv("MVX_BIND_FILL");
  if (bf) {
    int t = -1, a = -1;
    std::sscanf(bf, "%d,%d", &t, &a);
    hipStream_t st = ctx().main.stream;
    if (t >= 0) HIPCHECK(hipMemsetAsync(v.T, t & 255, L.o_bvar - L.o_T, st));
    if (a >= 0) HIPCHECK(hipMemsetAsync(v.bvar, a & 255, L.total - L.o_bvar, st));
  }
}

static const size_t SLAB_CACHE_LIMIT = (size_t)32 << 30; // idle bytes kept for reuse (of 288 GB)

// caller holds the cache lock.  Give idle memory back to the driver: every idle slab that is not part of an arena, and
// every arena whose slabs are all idle; stops once the idle bytes are at or below `keep`.
static void slab_trim(SlabCache &sc, size_t keep) {
  if (sc.idle_bytes <= keep) return;
  (void)hipDeviceSynchronize(); // queued work may still read a slab that was recycled a moment ago
  for (auto it = sc.free_slabs.begin(); it != sc.free_slabs.end() && sc.idle_bytes > keep;) {
    if (sc.arena_of.count(it->second)) {
      ++it;
      continue;
    }
    (void)hipFree(it->second);
    sc.idle_bytes -= it->first;
    it = sc.free_slabs.erase(it);
  }
  for (size_t a = 0; a < sc.arenas.size() && sc.idle_bytes > keep; a++) {
    Arena &ar = sc.arenas[a];
    if (!ar.base || ar.idle != ar.count) continue;
    auto range = sc.free_slabs.equal_range(ar.slab_bytes);
    for (auto it = range.first; it != range.second;) {
      auto f = sc.arena_of.find(it->second);
      if (f != sc.arena_of.end() && f->second == (int)a) {
        sc.arena_of.erase(f);
        it = sc.free_slabs.erase(it);
      } else
        ++it;
    }
    (void)hipFree(ar.base);
    sc.idle_bytes -= ar.slab_bytes * (size_t)ar.count;
    ar.base = nullptr;
  }
}

// Fresh device memory is not zeroed by the driver (it holds whatever the last process left there), and a slab has
// regions no kernel of a solve writes before the first whole-slab clone reads them (spare rows for cuts, the padding of
// a row, array tails): they are never part of a result, but they travel with every clone, so they start as zeros.
// MVX_SLAB_FILL=<byte> fills with that byte instead (255: NaN patterns, to flush out a read of such a region).
static void slab_fill(void *p, size_t bytes) {
  static hipStream_t fill_stream = nullptr;
  static const int fill = std::getenv("MVX_SLAB_FILL") ? std::atoi(std::getenv("MVX_SLAB_FILL")) : 0;
  if (fill < 0) return;
  if (!fill_stream) HIPCHECK(hipStreamCreateWithFlags(&fill_stream, hipStreamNonBlocking));
  HIPCHECK(hipMemsetAsync(p, fill & 255, bytes, fill_stream));
  HIPCHECK(hipStreamSynchronize(fill_stream));
}

// nullptr when the device is out of memory even after the idle slabs have been given back (mvx_last_error() then
// reads MVX_ENOMEM); never aborts
static void *slab_alloc(Context &c, size_t bytes) {
  SlabCache &sc = c.slabs;
  std::lock_guard<std::mutex> lk(sc.mu);
  auto it = sc.free_slabs.find(bytes);
  if (it != sc.free_slabs.end()) {
    void *p = it->second;
    sc.free_slabs.erase(it);
    sc.idle_bytes -= bytes;
    auto f = sc.arena_of.find(p);
    if (f != sc.arena_of.end()) sc.arenas[(size_t)f->second].idle--;
    return p;
  }
  void *p = nullptr;
  if (bytes <= ((size_t)64 << 20)) {
    // A size class doubles each time it runs dry (32, 32, 64, 128, ... slabs, at most 16 GB at once): a B&B frontier of
    // a thousand 4 MB node tableaux is six allocations, not thirty.  hipMalloc beside two threads that launch and wait
    // was measured at 60-130 us per CLONE in arenas of 32 (milliseconds per call), against 12 us when the process is idle.
    const size_t least = std::min<size_t>(32, std::max<size_t>(2, ((size_t)256 << 20) / bytes));
    size_t have = 0;
    for (const Arena &ar : sc.arenas)
      if (ar.base && ar.slab_bytes == bytes) have += (size_t)ar.count;
    size_t count = std::min(std::max(least, have), std::max<size_t>(least, ((size_t)16 << 30) / bytes));
    if (hipMalloc(&p, bytes * count) != hipSuccess) {
      (void)hipGetLastError();
      count = least;
      p = nullptr;
      if (hipMalloc(&p, bytes * count) != hipSuccess) p = nullptr;
    }
    if (p) {
      slab_fill(p, bytes * count);
      Arena ar;
      ar.base = p;
      ar.slab_bytes = bytes;
      ar.count = (int)count;
      ar.idle = (int)count - 1;
      const int a = (int)sc.arenas.size();
      sc.arenas.push_back(ar);
      for (size_t k = 0; k < count; k++) {
        void *q = (unsigned char *)p + k * bytes;
        sc.arena_of.emplace(q, a);
        if (k) sc.free_slabs.emplace(bytes, q);
      }
      sc.idle_bytes += bytes * (count - 1);
      return p;
    }
    (void)hipGetLastError();
    p = nullptr;
  }
  if (hipMalloc(&p, bytes) == hipSuccess) {
    slab_fill(p, bytes);
    return p;
  }
  (void)hipGetLastError();
  slab_trim(sc, 0); // give everything idle back and retry once
  if (hipMalloc(&p, bytes) == hipSuccess) {
    slab_fill(p, bytes);
    return p;
  }
  (void)hipGetLastError();
  g_last_error.store(MVX_ENOMEM);
  return nullptr;
}

// back to the cache (the streams are in order: work already queued on the slab finishes before any reuse)
static void slab_recycle(Context &c, void *slab, size_t bytes) {
  SlabCache &sc = c.slabs;
  std::lock_guard<std::mutex> lk(sc.mu);
  auto f = sc.arena_of.find(slab);
  if (f != sc.arena_of.end()) sc.arenas[(size_t)f->second].idle++;
  sc.free_slabs.emplace(bytes, slab);
  sc.idle_bytes += bytes;
  if (sc.idle_bytes > SLAB_CACHE_LIMIT) slab_trim(sc, SLAB_CACHE_LIMIT / 2);
}

void release_device(mvx_prob *P) {
  if (!P->slab) return;
  Context &c = ctx();
  {
    MAIN_LOCK(c);
    // a recorded clone still reads from / writes to this slab: launch it before the slab can be handed out again
    const unsigned char *lo = (const unsigned char *)P->slab, *hi = lo + P->slab_bytes;
    for (const CopyJob &j : c.copies)
      if (((const unsigned char *)j.src >= lo && (const unsigned char *)j.src < hi) ||
          ((const unsigned char *)j.dst >= lo && (const unsigned char *)j.dst < hi)) {
        flush_copies(c);
        break;
      }
  }
  slab_recycle(c, P->slab, P->slab_bytes);
  P->slab = nullptr;
  P->slab_bytes = 0;
  P->d_T = nullptr;
  P->valid = false;
}

static bool alloc_device(mvx_prob *P, int m_cap, int ld) {
  Context &c = ctx();
  SlabLayout L = slab_layout(m_cap, ld);
  void *slab = slab_alloc(c, L.total);
  if (!slab) return false;
  bind_slab(P, slab, m_cap, ld);
  return true;
}

static int ld_for(int n) { return (int)align_up((size_t)n + 1, LD_ALIGN); }

// A handle on its way to a slab of another geometry (DESIGN.md "Live edits").  slab_move binds the new slab and hands back
// the view the device work reads (`from`, the old slab) and the one it writes (`to`); both are the handle's own view when the
// geometry is the one it has.  Once that work is queued, slab_move_done recycles the old slab behind it (in-order stream: the
// work completes before any reuse).  false: the device is out of memory, the handle is left as it was.
struct SlabMove {
  SlabView from, to;
  void *old_slab = nullptr;
  size_t old_bytes = 0;
};
static bool slab_move(Context &c, mvx_prob *P, int m_cap, int ld, SlabMove &mv) {
  mv.from = mv.to = slab_view(P);
  if (m_cap == P->m_cap && ld == P->ld) return true;
  void *slab = slab_alloc(c, slab_layout(m_cap, ld).total);
  if (!slab) return false;
  mv.old_slab = P->slab;
  mv.old_bytes = P->slab_bytes;
  bind_slab(P, slab, m_cap, ld);
  mv.to = slab_view(P);
  return true;
}
static void slab_move_done(Context &c, SlabMove &mv) {
  if (mv.old_slab) slab_recycle(c, mv.old_slab, mv.old_bytes);
  mv.old_slab = nullptr;
}

// grow row capacity, preserving contents; false (handle left as it was) when the device is out of memory
static bool grow_rows(mvx_prob *P, int m_new) {
  if (m_new + ROW_SPARE <= P->m_cap) return true;
  Context &c = ctx();
  MAIN_LOCK(c);
  flush_copies(c);
  hipStream_t st = c.main.stream;
  const size_t rows = (size_t)P->m_cap + 1, ld = (size_t)P->ld;
  SlabMove mv;
  if (!slab_move(c, P, m_new + ROW_SLACK, P->ld, mv)) return false;
  const SlabView &o = mv.from, &v = mv.to;
  HIPCHECK(hipMemcpyAsync(v.T, o.T, rows * ld * 8, hipMemcpyDeviceToDevice, st));
  HIPCHECK(hipMemcpyAsync(v.bvar, o.bvar, rows * 4, hipMemcpyDeviceToDevice, st));
  HIPCHECK(hipMemcpyAsync(v.blb, o.blb, rows * 8, hipMemcpyDeviceToDevice, st));
  HIPCHECK(hipMemcpyAsync(v.bub, o.bub, rows * 8, hipMemcpyDeviceToDevice, st));
  HIPCHECK(hipMemcpyAsync(v.nvar, o.nvar, ld * 4, hipMemcpyDeviceToDevice, st));
  HIPCHECK(hipMemcpyAsync(v.nflag, o.nflag, ld * 4, hipMemcpyDeviceToDevice, st));
  HIPCHECK(hipMemcpyAsync(v.nlb, o.nlb, ld * 8, hipMemcpyDeviceToDevice, st));
  HIPCHECK(hipMemcpyAsync(v.nub, o.nub, ld * 8, hipMemcpyDeviceToDevice, st));
  slab_move_done(c, mv);
  return true;
}

// --------------------------------------------------------------------------- helpers
static inline double nb_value(int flag, double lb, double ub) {
  switch (flag) {
    case MVX_NL: return lb;
    case MVX_NU: return ub;
    case MVX_NS: return lb;
    default: return 0.0;
  }
}
static inline int std_flag(int type) {
  switch (type) {
    case MVX_FR: return MVX_NF;
    case MVX_LO: return MVX_NL;
    case MVX_UP: return MVX_NU;
    case MVX_DB: return MVX_NL;
    default: return MVX_NS;
  }
}

static void rebuild_pos(mvx_prob *P) {
  P->pos.assign((size_t)P->m + P->n + 1, 0);
  for (int i = 1; i <= P->m; i++) P->pos[P->bvar[i]] = i;
  for (int j = 1; j <= P->n; j++) P->pos[P->nvar[j]] = -j;
}

// variable-indexed bounds from the model
static inline void var_bounds(const mvx_prob *P, int k, double *lb, double *ub) {
  if (k <= P->m) {
    *lb = P->rlb[k];
    *ub = P->rub[k];
  } else {
    *lb = P->clb[k - P->m];
    *ub = P->cub[k - P->m];
  }
}

// Cluster selection (k_chain): one launch chooses a whole chain.  MVX_CLUSTER=0 keeps the two launches per step
// (k_pc / k_pr), which also take over for the rest of the process when a cluster launch ever gives up waiting for its
// peer workgroups (cl_abort), and serve the geometries k_chain does not cover (more than 16384 rows or columns).
static std::atomic<int> g_cluster{-1};
static std::atomic<bool> g_cluster_broken{false};
static std::atomic<long long> g_cluster_launches{0}, g_cluster_aborts{0};
static bool cluster_wanted() {
  int v = g_cluster.load();
  if (v < 0) {
    const char *e = std::getenv("MVX_CLUSTER");
    v = e ? (std::atoi(e) != 0) : 1;
    g_cluster.store(v);
  }
  return v != 0 && !g_cluster_broken.load();
}

// Steps per bulk launch of the chained primal path.  A step costs two small launches (k_pc / k_pr) or its share of one
// k_chain launch, a pass over the tableau costs its bytes: chains pay at every size, the longer the pass the longer the
// chain (scripts/chainsweep.py).
// MVX_CHAIN=1 turns the chaining off, 2..KCH fixes the length.
static int g_chain = -1;
static int chain_length(const mvx_prob *P) {
  if (g_chain < 0) {
    const char *e = std::getenv("MVX_CHAIN");
    g_chain = e ? std::max(1, std::min(KCH, std::atoi(e))) : 0;
  }
  if (g_chain > 0) return g_chain;
  const size_t bytes = (size_t)(P->m + 1) * (size_t)P->ld * 8;
  if (cluster_wanted() && chain_cluster_kmax(P->m, P->n) > 0) return bytes < ((size_t)24 << 20) ? 16 : 32; // a step costs no launch there
  if (bytes < ((size_t)24 << 20)) return 8;
  return 16;
}

// Dual pivots one k_update applies (dual_chain; MVX_DCHAIN=1 turns it off, 2..8 fixes the length).  The chain is built
// inside k_select at a few microseconds per step; what it saves is the k_update pass and the two launch boundaries of
// every step it absorbs.  Where the pass is the cost -- a launch shared by many node LPs, or one large tableau -- the
// longest chain pays (wide 512x1024 tree: 9.1 k nodes/s unchained, 14.8 k at 4, 18.9 k at 8); where a few small
// tableaux wait on each other's longest solve, 4 is the optimum (config-5 tree: 3.30 k, 4.40 k at 4, 4.22 k at 8).
static int g_dchain = -1;
static int dual_chain_length(bool wide, bool on_chip = false) {
  if (g_dchain < 0) {
    const char *e = std::getenv("MVX_DCHAIN");
    g_dchain = e ? std::max(1, std::min(DCH_MAX, std::atoi(e))) : 0;
  }
  if (g_dchain > 0) return g_dchain;
  // node LPs that k_dsel takes (up to 1024 x 1024): a chained step costs a few microseconds there, the longest chain pays
  // (config-5 tree: 5.5 k nodes/s at 4, 5.8 k at 6 and 8; wide tree 158 -> 140 ms per 2000 nodes)
  if (on_chip) return 8;
  return wide ? 8 : 4;
}

// No limit asked for: a safety cap stands in (belt and braces behind the anti-cycling rule; a stalled
// degenerate LP must end with EITLIM rather than spin on the device).  Same formula as the oracle.
static int pivot_budget(const mvx_prob *P, const mvx_smcp &parm) {
  return parm.it_lim >= 0 ? parm.it_lim : 200 * (P->m + P->n) + 100000;
}

// The handle's part of a fresh control block, the same for a single solve (fill_ctl) and a job of a batch (batch_fill_job):
// everything else is zero, the scratch pointers and chain lengths are the caller's.
static void ctl_for_handle(Ctl *h, const mvx_prob *P, double tol_bnd, double tol_dj, double tol_piv, int budget) {
  std::memset(h, 0, sizeof(Ctl));
  h->T = P->d_T;
  h->bvar = P->d_bvar; h->blb = P->d_blb; h->bub = P->d_bub;
  h->nvar = P->d_nvar; h->nflag = P->d_nflag; h->nlb = P->d_nlb; h->nub = P->d_nub;
  h->m = P->m; h->n = P->n; h->ld = P->ld; h->m_cap = P->m_cap;
  h->sgn = (P->dir == MVX_MAX) ? 1.0 : -1.0;
  h->tol_bnd = tol_bnd; h->tol_dj = tol_dj; h->tol_piv = tol_piv;
  h->phase = PH_START; h->done = D_RUN; h->budget = budget;
  h->stall = 0; h->stall_limit = g_stall_limit > 0 ? g_stall_limit : 64 + (P->m + P->n) / 8;
  h->fstate = F_OFF;
  h->nch = 1;
}

// control block of a launch sequence on `sc`.  Without parm (mirror exports, tableau refresh, model edits): tolerances 1e-9,
// no pivot budget
static void fill_ctl(SolveCtx &sc, mvx_prob *P, Ctl *h, const mvx_smcp *parm = nullptr) {
  if (parm) ctl_for_handle(h, P, parm->tol_bnd, parm->tol_dj, parm->tol_piv, pivot_budget(P, *parm));
  else ctl_for_handle(h, P, 1e-9, 1e-9, 1e-9, -1);
  h->colq = sc.d_colq; h->srow = sc.d_srow; h->cost1 = sc.d_cost1; h->wts = sc.d_wts;
  h->gflag = sc.d_gflag; h->part = sc.d_part; h->rc_base = nullptr; h->rc_out = sc.d_cost1;
  h->olb = sc.d_olb; h->oub = sc.d_oub; h->dw = sc.d_dw;
  h->dwx[0] = sc.d_dw; h->dwx[1] = sc.d_dw2;
  h->pw[0] = sc.d_pw[0]; h->pw[1] = sc.d_pw[1];
  h->p1_list = sc.d_p1list;
  h->colqx[0] = sc.d_colqx[0]; h->colqx[1] = sc.d_colqx[1];
  h->betac[0] = sc.d_betac[0]; h->betac[1] = sc.d_betac[1];
  h->pp[0] = sc.d_pp[0]; h->pp[1] = sc.d_pp[1]; h->rp = sc.d_rp;
  h->npb = fused_npb(P->n); h->nrb = 0; // nrb is published by k_fb (its grid height)
  for (int k = 0; k < KCH; k++) {
    h->srowk[k] = sc.d_srowk[k];
    h->colqk[k] = sc.d_colqk[k];
  }
  h->pc_epoch = 1;
  {
    static unsigned long long *dbg = nullptr;
    static bool looked = false;
    if (!looked) {
      looked = true;
      if (std::getenv("MVX_FCS_DBG")) {
        HIPCHECK(hipMalloc((void **)&dbg, (size_t)KCH * 16 * 8));
        HIPCHECK(hipMemset(dbg, 0, (size_t)KCH * 16 * 8));
        HIPCHECK(hipDeviceSynchronize());
      }
    }
    h->dbg = dbg;
  }
  h->rpc = sc.d_rpc;
  h->chain_max = chain_length(P);
  h->dchain_max = dual_chain_length((size_t)(P->m + 1) * (size_t)P->ld * 8 >= ((size_t)16 << 20), P->m <= 1024 && P->n <= 1024);
}

// the handle's pending bound edits ride in the control block of the solve that is about to start
static void take_edits(mvx_prob *P, Ctl *h) {
  h->n_edits = (int)P->pending.size();
  for (int k = 0; k < h->n_edits; k++) {
    h->edit_row[k] = P->pending[(size_t)k].row;
    h->edit_lb[k] = P->pending[(size_t)k].lb;
    h->edit_ub[k] = P->pending[(size_t)k].ub;
  }
  P->pending.clear();
}

// ... or go to the device now (more than MAX_EDITS of them, or something other than a solve needs the bounds there)
static void flush_edits(SolveCtx &sc, mvx_prob *P) {
  for (const auto &e : P->pending) launch_set_basic_bounds(P->d_blb, P->d_bub, e.row, e.lb, e.ub, sc.stream);
  P->pending.clear();
}

static void upload_ctl(SolveCtx &sc) {
  HIPCHECK(hipMemcpyAsync(sc.d_ctl, sc.h_ctl, sizeof(Ctl), hipMemcpyHostToDevice, sc.stream));
}

// the basis / solution mirrors an export packed into a staging area become the handle's
static void publish_mirrors(mvx_prob *P, const StageView &v) {
  P->beta.assign(v.beta, v.beta + P->m + 1);
  P->dj.assign(v.dj, v.dj + P->n + 1);
  P->bvar.assign(v.bvar, v.bvar + P->m + 1);
  P->nvar.assign(v.nvar, v.nvar + P->n + 1);
  P->nflag.assign(v.nflag, v.nflag + P->n + 1);
  rebuild_pos(P);
  P->sol_fresh = true;
  P->fresh_rows = -1;
}

// copy the staging buffer back and refresh the host mirrors
static void pull_stage(SolveCtx &sc, mvx_prob *P, bool mirrors) {
  if (!sc.stage_zc) HIPCHECK(hipMemcpyAsync(sc.h_stage, sc.d_stage, StageView::bytes(P->m_cap, P->ld), hipMemcpyDeviceToHost, sc.stream));
  HIPCHECK(hipStreamSynchronize(sc.stream));
  if (mirrors) publish_mirrors(P, StageView(sc.h_stage, P->m_cap, P->ld));
}

void refresh_solution(const mvx_prob *Pc) {
  mvx_prob *P = const_cast<mvx_prob *>(Pc);
  if (!P->valid || P->sol_fresh) return;
  Context &c = ctx();
  bind_device(c);
  MAIN_LOCK(c);
  flush_copies(c);
  SolveCtx &sc = c.main;
  ensure_scratch(sc, P->m_cap, P->ld);
  fill_ctl(sc, P, sc.h_ctl);
  upload_ctl(sc);
  launch_export(sc.d_ctl, sc.d_stage, P->m, P->n, 1, sc.stream);
  pull_stage(sc, P, true);
}

// ---------------------------------------------------------------------- tableau build
// false: the device is out of memory (mvx_last_error() reads MVX_ENOMEM); the handle stays without a tableau
static bool build_slack_tableau(mvx_prob *P, const int *sflag = nullptr) { // sflag: non-basic status per structural column (refresh)
  Context &c = ctx();
  MAIN_LOCK(c);
  SolveCtx &sc = c.main;
  const int m = P->m, n = P->n;
  const int ld = ld_for(n);
  if (P->slab && (P->ld != ld || P->m_cap < m + ROW_SPARE)) release_device(P);
  if (!P->slab && !alloc_device(P, m + ROW_SLACK, ld)) {
    P->status = MVX_UNDEF;
    return false;
  }
  ensure_scratch(sc, P->m_cap, P->ld);
  P->bvar.assign((size_t)m + 1, 0);
  P->nvar.assign((size_t)n + 1, 0);
  P->nflag.assign((size_t)n + 1, 0);
  std::vector<double> nlb((size_t)ld, 0.0), nub((size_t)ld, 0.0), blb((size_t)m + 1, 0.0), bub((size_t)m + 1, 0.0);
  std::vector<double> xn((size_t)n + 1, 0.0);
  bool any_x = false;
  for (int j = 1; j <= n; j++) {
    P->nvar[j] = m + j;
    P->nflag[j] = sflag ? sflag[j] : std_flag(P->ctype[j]);
    nlb[j] = P->clb[j];
    nub[j] = P->cub[j];
    xn[j] = nb_value(P->nflag[j], nlb[j], nub[j]);
    any_x = any_x || xn[j] != 0.0;
  }
  for (int i = 1; i <= m; i++) {
    P->bvar[i] = i;
    blb[i] = P->rlb[i];
    bub[i] = P->rub[i];
  }
  // host tableau, uploaded row by row through a pinned bounce buffer
  const size_t rows_per_chunk = std::max<size_t>(1, ((size_t)32 << 20) / ((size_t)ld * 8));
  double *bounce = nullptr;
  HIPCHECK(hipHostMalloc((void **)&bounce, rows_per_chunk * ld * 8));
  for (size_t r0 = 0; r0 <= (size_t)m; r0 += rows_per_chunk) {
    size_t r1 = std::min<size_t>((size_t)m + 1, r0 + rows_per_chunk);
    for (size_t i = r0; i < r1; i++) {
      double *row = bounce + (i - r0) * ld;
      std::memset(row, 0, (size_t)ld * 8);
      if (i == 0) {
        double z = P->c[0];
        for (int j = 1; j <= n; j++) {
          row[j] = P->c[j];
          if (xn[j] != 0.0) z = std::fma(P->c[j], xn[j], z);
        }
        row[0] = z;
      } else {
        const double *a = P->A[i]->data();
        std::memcpy(row + 1, a + 1, (size_t)n * 8);
        double acc = 0.0;
        if (any_x)
          for (int j = 1; j <= n; j++)
            if (xn[j] != 0.0) acc = std::fma(a[j], xn[j], acc);
        row[0] = acc;
      }
    }
    HIPCHECK(hipMemcpyAsync(P->d_T + r0 * ld, bounce, (r1 - r0) * ld * 8, hipMemcpyHostToDevice, sc.stream));
    HIPCHECK(hipStreamSynchronize(sc.stream));
  }
  HIPCHECK(hipHostFree(bounce));
  HIPCHECK(hipMemcpyAsync(P->d_bvar, P->bvar.data(), (size_t)(m + 1) * 4, hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipMemcpyAsync(P->d_blb, blb.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipMemcpyAsync(P->d_bub, bub.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice, sc.stream));
  std::vector<int> nv((size_t)ld, 0), nf((size_t)ld, MVX_NS);
  for (int j = 1; j <= n; j++) {
    nv[j] = P->nvar[j];
    nf[j] = P->nflag[j];
  }
  HIPCHECK(hipMemcpyAsync(P->d_nvar, nv.data(), (size_t)ld * 4, hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipMemcpyAsync(P->d_nflag, nf.data(), (size_t)ld * 4, hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipMemcpyAsync(P->d_nlb, nlb.data(), (size_t)ld * 8, hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipMemcpyAsync(P->d_nub, nub.data(), (size_t)ld * 8, hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipStreamSynchronize(sc.stream));
  rebuild_pos(P);
  P->pending.clear(); // the bounds just uploaded are the model's
  P->valid = true;
  P->sol_fresh = false;
  P->fresh_rows = -1;
  P->status = MVX_UNDEF;
  return true;
}

// ------------------------------------------------------------------------------ simplex
static void flush_update_events(Context &c, size_t used) {
  for (size_t k = 0; k + 1 < used; k += 2) {
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, c.ev_pool[k], c.ev_pool[k + 1]));
    c.prof_update_ms += ms;
    c.prof_update_n++;
  }
}

// A solve is a small host-side state machine around queued launches, so that several of them
// can be in flight on different streams (engine_simplex_batch): begin -> {enqueue, sync, collect}*.
// ---- resident-tableau path (k_persist): which problems take it, its buffers, backup and restore
constexpr int PERSIST_HEAD_STRIDE_MAX = 4; // granules between two strips' heads
static std::atomic<int> g_persist_mode{-1}; // -1: environment MVX_PERSIST (default on), 0 off, 1 on
static std::atomic<bool> g_persist_broken{false}; // a launch aborted (its workgroups were not co-resident in time): off for good
static std::atomic<long long> g_persist_launches{0}, g_persist_aborts{0};
struct PersistPlan {
  int cpw = 0, nw = 0;
  size_t lds = 0;
};
static bool persist_plan(Context &c, const mvx_prob *P, PersistPlan *pl) {
  if (g_persist_broken) return false;
  if (g_persist_mode < 0) {
    const char *e = std::getenv("MVX_PERSIST");
    g_persist_mode = (e && e[0] == '0') ? 0 : ((e && e[0] == '2') ? 2 : 1);
  }
  if (!g_persist_mode) return false;
  static int cus = 0;
  if (!cus) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.dev) != hipSuccess) return false;
    cus = prop.multiProcessorCount;
  }
  const int m = P->m, n = P->n;
  if ((long)(m + 1) * (n + 1) < 32768) return false; // a handful of pivots: the launch is not worth its set-up
  // Measured (profiles/r02_persist_ab.jsonl): 256x512 29.6 -> 10.6 us/pivot, 512x1024 16.0 -> 12.1, 1024x2048 15.9 -> 15.6,
  // 1024x4096 20.3 -> 20.2: the per-pivot gather of the 256 proposals costs ~6.5 us whatever the size (3.6 polling sweeps
  // of ~1.8 us each), the strip work grows with m.  MVX_PERSIST=2 lifts the size cap for experiments.
  if (g_persist_mode < 2 && (long)(m + 1) * (n + 1) > 700000) return false;
  const int cpw = (n + cus - 1) / cus;
  if (cpw > persist_max_cpw()) return false;
  pl->cpw = cpw;
  pl->nw = (n + cpw - 1) / cpw; // one workgroup per CU at most: every workgroup must be resident at once
  if (pl->nw > 256) return false; // the exchange buffers are sized for 256 workgroups
  pl->lds = persist_lds_bytes(m, cpw);
  return pl->lds <= (size_t)150 * 1024;
}

static bool ensure_persist(Context &c, SolveCtx &sc, const mvx_prob *P) {
  const int words = persist_slot_words(P->m_cap);
  if (!sc.d_pabort) {
    HIPCHECK(hipMalloc((void **)&sc.d_pabort, 1024));
    HIPCHECK(hipMemsetAsync(sc.d_pabort, 0, 1024, sc.stream));
    HIPCHECK(hipHostMalloc((void **)&sc.h_pabort, 1024));
    sc.h_pabort[0] = 0;
    HIPCHECK(hipMalloc((void **)&sc.d_pcand, (size_t)2 * 256 * PERSIST_HEAD_STRIDE_MAX * 8));
    HIPCHECK(hipMalloc((void **)&sc.d_pctl, sizeof(Ctl)));
  }
  if (words > sc.p_msg_words) {
    HIPCHECK(hipStreamSynchronize(sc.stream));
    if (sc.d_pmsg) HIPCHECK(hipFree(sc.d_pmsg));
    HIPCHECK(hipMalloc((void **)&sc.d_pmsg, (size_t)2 * 256 * words * 8)); // a slot per workgroup and parity
    sc.p_msg_words = words;
  }
  if (P->ld > sc.p_pw_ld) {
    HIPCHECK(hipStreamSynchronize(sc.stream));
    if (sc.d_ppw) HIPCHECK(hipFree(sc.d_ppw));
    HIPCHECK(hipMalloc((void **)&sc.d_ppw, (size_t)2 * P->ld * 8));
    sc.p_pw_ld = P->ld;
  }
  if (sc.p_backup_bytes != P->slab_bytes) {
    if (sc.p_backup) slab_recycle(c, sc.p_backup, sc.p_backup_bytes);
    sc.p_backup = slab_alloc(c, P->slab_bytes);
    sc.p_backup_bytes = sc.p_backup ? P->slab_bytes : 0;
    if (!sc.p_backup) {
      (void)g_last_error.exchange(0); // not an error of the caller's: the two-kernel path serves
      return false;
    }
  }
  return true;
}

struct SolveJob {
  mvx_prob *P = nullptr;
  SolveCtx *sc = nullptr;
  mvx_smcp parm;
  enum { MAIN, PHASE1, FINAL } mode = MAIN;
  int batch = 8, pb = 4;
  int done = D_RUN;
  bool try_fused = false;
  bool try_dfused = false;    // dual phase on a large tableau: k_dboot / k_da / k_fb<DUAL>
  bool persist_queued = false; // this batch of launches contains a k_persist launch (its abort flag is copied back)
  int seen_steps = 0, seen_pivots = 0, seen_bulk = 0;
  int chain = 1, chain0 = 1; // pivots per bulk launch the next batch is queued for / the size rule's choice
  bool resident = false;     // this solve holds the token that lets it launch kernels whose workgroups must be resident together
  bool cluster = false;      // the chains of this solve are chosen by k_chain (one launch) instead of k_pc / k_pr per step
  ChainArgs cargs{};         // what the kernels of the chained primal path take by value
  size_t ev_used = 0;
  bool profiled = false;
  int rc = 0;
  Ctl snap;
};

static void stage_copy_async(SolveCtx &sc, const mvx_prob *P) {
  HIPCHECK(hipEventRecord(sc.ev_b, sc.stream)); // end of the device work queued so far (last_solve_ms)
  if (!sc.stage_zc) HIPCHECK(hipMemcpyAsync(sc.h_stage, sc.d_stage, StageView::bytes(P->m_cap, P->ld), hipMemcpyDeviceToHost, sc.stream));
  if (sc.d_pabort) HIPCHECK(hipMemcpyAsync(sc.h_pabort, sc.d_pabort, 512, hipMemcpyDeviceToHost, sc.stream)); // abort flag + phase cycle totals
}

// The fused dual pipeline replaces k_select's four dependent stages (34 us at 4096x8192) by k_da (~8 us); below about
// two million tableau entries the update itself is so short that the two extra bootstrap launches do not pay.
static std::atomic<int> g_dual_fused{-1}; // 0 never, 1 size rule (default), 2 always; -1: MVX_DUAL_FUSED not read yet
static std::atomic<long long> g_dfused_boots{0}, g_dfused_pivots{0};
static bool dual_fused_worth_it(const mvx_prob *P) {
  int mode = g_dual_fused.load();
  if (mode < 0) {
    const char *e = std::getenv("MVX_DUAL_FUSED");
    const int v = e ? std::atoi(e) : 1;
    mode = v < 0 ? 1 : std::min(2, v);
    g_dual_fused.store(mode);
  }
  if (mode == 0) return false;
  if (mode >= 2) return true;
  // ... and from about twelve million entries on the generic path with its dual pivots chained eight to a pass is the
  // faster one (4096x8192: 67.7 against 96.5 us per dual pivot; 2048x4096: 40.4 against 39.9, scripts/dualtime.py)
  const long entries = (long)(P->m + 1) * (P->n + 1);
  return entries >= 2000000 && entries < 12000000;
}

static void job_begin(Context &c, SolveJob &J) {
  mvx_prob *P = J.P;
  SolveCtx &sc = *J.sc;
  ensure_scratch(sc, P->m_cap, P->ld);
  Ctl *h = sc.h_ctl;
  fill_ctl(sc, P, h, &J.parm);
  take_edits(P, h);
  upload_ctl(sc);
  HIPCHECK(hipEventRecord(sc.ev_a, sc.stream));
  {
    ChainArgs &a = J.cargs;
    a.c = sc.d_ctl;
    a.T = P->d_T;
    a.blb = P->d_blb; a.bub = P->d_bub; a.nlb = P->d_nlb; a.nub = P->d_nub; a.nflag = P->d_nflag;
    a.betab = sc.d_betab;
    for (int k = 0; k < 2; k++) {
      a.pw[k] = sc.d_pw[k];
      a.drowk[k] = sc.d_drowk[k]; a.pwk[k] = sc.d_pwk[k]; a.nlbk[k] = sc.d_nlbk[k]; a.nubk[k] = sc.d_nubk[k]; a.nflagk[k] = sc.d_nflagk[k];
      a.betak[k] = sc.d_betak[k]; a.blbk[k] = sc.d_blbk[k]; a.bubk[k] = sc.d_bubk[k];
    }
    a.pp = sc.d_ppart; a.rp = sc.d_rpart; a.ppstride = sc.pp_stride; a.rpstride = sc.rp_stride;
    a.srow0 = sc.d_srowk[0]; a.colq0 = sc.d_colqk[0];
    a.sstride = sc.sk_stride; a.cstride = sc.ck_stride;
    a.m = P->m; a.n = P->n; a.ld = P->ld; a.mcap1 = P->m_cap + 1;
    a.ncb = chain_ncb(P->n); a.nrb = chain_nrb(P->m);
    a.tol_dj = h->tol_dj; a.tol_piv = h->tol_piv; a.tol_bnd = h->tol_bnd; a.sgn = h->sgn;
    a.stall_limit = h->stall_limit;
    a.zeros = sc.d_zeros;
    a.xg = sc.d_xg; a.xg_bytes = (int)XG_BYTES; a.xabort = sc.d_xabort;
    a.nw = chain_cluster_nw(P->m, P->n); a.kmax = 0; a.tagbase = 0; a.boot = 0;
  }
  // k_chain and k_persist need their workgroups resident together: two such launches from two host threads (the main
  // context and a B&B worker's) could each hold half of the CUs they both need and wait for the rest until they time
  // out.  One solve at a time may use them (solve_once holds the token for the length of the call); a solve that finds
  // the token taken runs on the plain kernels.
  J.cluster = J.resident && cluster_wanted() && chain_cluster_kmax(P->m, P->n) > 0;
  J.try_fused = !P->hint_dual; // dual-phase warm starts (B&B children) skip the primal fast path
  J.chain = J.chain0 = h->chain_max;
  J.try_dfused = P->hint_dual && dual_fused_worth_it(P);
  J.profiled = c.prof && J.sc == &c.main;
  // With a pivot limit the number of pivots wanted is known: queue them in one go (up to 256) instead of
  // growing the batch 8, 16, 32, ... -- every batch boundary costs a host round trip and a generic
  // (one-workgroup) selection step.  A primal fast-path solve that ends before the limit leaves no-op
  // launches of ~2 us behind; dual warm starts keep the cautious growth (they usually end after a few pivots).
  if (J.parm.it_lim > 8 && J.try_fused) J.batch = std::min(J.parm.it_lim, 256);
}

static void job_enqueue(Context &c, SolveJob &J) {
  mvx_prob *P = J.P;
  SolveCtx &sc = *J.sc;
  const int m = P->m, n = P->n;
  J.ev_used = 0;
  if (J.mode == SolveJob::FINAL) {
    launch_export(sc.d_ctl, sc.d_stage, m, n, 1, sc.stream); // forced export (state left by a host-side decision)
    stage_copy_async(sc, P);
    return;
  }
  if (J.mode == SolveJob::PHASE1) {
    // host-driven phase 1: per iteration head (signs, changed rows) -> cost-row fix -> select -> update;
    // the cost row is tableau row m+1, so the update grid reaches one row further
    for (int k = 0; k < J.pb; k++) {
      launch_p1_head(sc.d_ctl, sc.stream);
      launch_p1_fix(sc.d_ctl, n, sc.stream);
      launch_p1_select(sc.d_ctl, sc.stream);
      launch_update(sc.d_ctl, m + 1, n, sc.stream);
    }
    launch_export(sc.d_ctl, sc.d_stage, m, n, 0, sc.stream);
    stage_copy_async(sc, P);
    return;
  }
  const int batch = J.batch;
  if (J.profiled && c.ev_pool.size() < (size_t)2 * batch + 4) { // sized for the largest batch
    size_t old = c.ev_pool.size();
    c.ev_pool.resize((size_t)2 * batch + 4);
    for (size_t k = old; k < c.ev_pool.size(); k++) HIPCHECK(hipEventCreate(&c.ev_pool[k]));
  }
  // with a pivot limit, never queue more pivots than the limit still allows (+1 launch so that
  // k_select can observe the exhausted budget): keeps no-op launches out of profiles
  const int remaining = (J.parm.it_lim >= 0) ? std::max(0, J.parm.it_lim - J.seen_pivots) : (1 << 30);
  auto ev = [&]() {
    if (J.profiled) HIPCHECK(hipEventRecord(c.ev_pool[J.ev_used++], sc.stream));
  };
  // (replaying each batch as one captured hipGraph was measured: no gain -- the dispatch of small kernels is
  // bound by the command processor, not by the host -- and removed)
  int depth;
  if (J.try_fused) depth = std::max(0, std::min(batch, remaining)); // + the generic step that closes the batch, if the limit leaves it a pivot
  else depth = std::max(1, std::min(batch, remaining));
  if (J.try_fused) {
    PersistPlan pl;
    // the resident-tableau kernel serves where the cluster chain is not on offer (mvx_set_cluster(0), a cluster launch
    // that gave up): since round 3 the chain is the faster one at every size that fits k_persist (scripts/smalltime.py:
    // 512x1024 9.1 against 12.3 us per pivot, 128x256 9.7 against 10.8)
    if (depth > 0 && !J.profiled && J.resident && !(J.cluster && !g_cluster_broken.load()) && persist_plan(c, P, &pl) && ensure_persist(c, sc, P)) {
      // cache-resident size: one generic step settles the phase, then the whole run of primal pivots in ONE launch
      // with the tableau held in LDS.  In front of it a backup (slab, control block, both devex weight sets): a
      // launch whose workgroups do not all become resident in time aborts mid-step, and the backup is what the
      // two-kernel path then carries on from.
      launch_select(sc.d_ctl, sc.stream);
      launch_update(sc.d_ctl, m, n, sc.stream, 1, 1);
      HIPCHECK(hipMemcpyAsync(sc.p_backup, P->slab, P->slab_bytes, hipMemcpyDeviceToDevice, sc.stream));
      HIPCHECK(hipMemcpyAsync(sc.d_pctl, sc.d_ctl, sizeof(Ctl), hipMemcpyDeviceToDevice, sc.stream));
      HIPCHECK(hipMemcpyAsync(sc.d_ppw, sc.d_pw[0], (size_t)P->ld * 8, hipMemcpyDeviceToDevice, sc.stream));
      HIPCHECK(hipMemcpyAsync(sc.d_ppw + P->ld, sc.d_pw[1], (size_t)P->ld * 8, hipMemcpyDeviceToDevice, sc.stream));
      const int head_stride = 4; // 4 B .. 4 KB between heads measured the same
      HIPCHECK(hipMemsetAsync(sc.d_pcand, 0, (size_t)2 * pl.nw * head_stride * 8, sc.stream));
      const int steps = 1 << 24; // the pivot limit is the control block's `budget`, which the kernel counts down
      if (launch_persist(sc.d_ctl, sc.d_pcand, sc.d_pmsg, sc.d_pabort, (unsigned long long *)(sc.d_pabort + 16), P->m, pl.cpw, pl.nw, sc.p_msg_words, steps, head_stride, sc.stream) == 0) {
        J.persist_queued = true;
        g_persist_launches++;
        // what the run ended on (optimum, unbounded ray, stall, pivot limit) is settled by one generic step
        launch_select(sc.d_ctl, sc.stream);
        launch_update(sc.d_ctl, m, n, sc.stream, 1, 1);
      } else {
        g_persist_broken = true;
      }
    } else {
      // The fused two-kernel pipeline (k_fa / k_fb) first: k_fboot takes a call from its very first pivot when the
      // basis it starts from is primal feasible, and otherwise (dual simplex, phase 1, Bland's rule in force) turns
      // the pipeline off, so that its launches return at once.  One generic step closes the batch: it settles what
      // a stopped run ended on (optimum, unbounded ray, stall) in the same host round trip, and is an ordinary
      // pivot when nothing stopped.  Its events come first in the pool: the leading pairs are the ones that stepped.
      const size_t e_generic = J.ev_used;
      if (J.profiled) J.ev_used += 2;
      if (depth > 0) {
        // chained path: k_pboot once, then per chain of up to `kc` steps two small launches per step (k_pc / k_pr)
        // and one bulk launch (k_fbc3), so `depth` pivots take depth / kc passes over the tableau when every chain
        // fills (a chain that ends early leaves pivots for the next batch)
        const bool cl = J.cluster && !g_cluster_broken.load();
        if (!cl) launch_pboot(J.cargs, sc.stream); // k_chain does the start-of-batch checks itself (first launch: boot)
        bool first = true;
        const int kc = cl ? std::max(1, std::min(J.chain0, chain_cluster_kmax(m, n))) : std::max(1, J.chain);
        auto chain_launch = [&](int steps) { // k_chain: the whole selection of a chain of up to `steps` steps
          J.cargs.kmax = steps;
          J.cargs.boot = first ? 1 : 0;
          first = false;
          J.cargs.tagbase = sc.xtag;
          sc.xtag += 128;
          if (launch_chain(J.cargs, sc.stream) != 0) g_cluster_broken.store(true);
          g_cluster_launches++;
        };
        for (int left = depth; left > 0;) {
          const int steps = std::min(kc, left); // the last pass of a limited run chains only what the limit leaves
          if (cl) chain_launch(steps);
          else
            for (int t = 0; t < steps; t++) launch_pstep(J.cargs, t, sc.stream);
          ev(); // the profiled pair of events brackets the bulk launch: the pass and, beside it, the chain's patch jobs
          launch_fbc3(J.cargs, steps, sc.stream);
          ev();
          left -= steps;
        }
        // a run that may end on the pivot limit: one more selection, which finds the limit and reports it
        // (k_chain notes it itself when the limit falls on the end of its last chain: pc_itlim)
        if (J.parm.it_lim >= 0 && depth >= remaining && !cl) launch_pc(J.cargs, 0, sc.stream);
      }
      launch_select(sc.d_ctl, sc.stream);
      if (J.profiled) HIPCHECK(hipEventRecord(c.ev_pool[e_generic], sc.stream));
      launch_update(sc.d_ctl, m, n, sc.stream, 1, 1);
      if (J.profiled) HIPCHECK(hipEventRecord(c.ev_pool[e_generic + 1], sc.stream));
    }
  } else if (J.try_dfused) {
    // one generic step settles the phase (and restarts the dual devex weights when the phase has just been
    // entered); if it is the dual simplex, the fused pair k_da / k_fb<DUAL> takes over, otherwise its launches
    // return at once
    launch_select(sc.d_ctl, sc.stream);
    launch_update(sc.d_ctl, m, n, sc.stream, 1, 1);
    if (depth > 1) {
      launch_dboot(sc.d_ctl, n, sc.stream);
      launch_db(sc.d_ctl, m, n, sc.stream);
      for (int k = 0; k < depth - 1; k++) {
        launch_da(sc.d_ctl, n, sc.stream);
        launch_db(sc.d_ctl, m, n, sc.stream);
      }
    }
  } else {
    for (int k = 0; k < depth; k++) {
      launch_dsel(sc.d_ctl, m, n, sc.stream); // a dual phase carrying on (warm starts): the chain on chip, k_select then returns
      launch_select(sc.d_ctl, sc.stream);
      ev();
      launch_update(sc.d_ctl, m, n, sc.stream, 1, 1);
      ev();
    }
  }
  launch_export(sc.d_ctl, sc.d_stage, m, n, 0, sc.stream);
  stage_copy_async(sc, P);
}

// What a solve that has ended reports on its handle, for a single solve and a job of a batch alike: the counters of the
// control block `snap` it ended with, and status and return code by `done` -- the single path's own verdict (D_FAIL after
// 64 phase-1 rounds) or the snapshot's.  Returns the code.
static int book_result(mvx_prob *P, const Ctl &snap, int done, double last_ms) {
  P->it_cnt += snap.it_cnt;
  P->bland_cnt += snap.n_bland;
  P->pert_cnt += snap.n_pert;
  g_dfused_boots += snap.n_dboot; // counted by the lead threads of k_dboot / k_fb<DUAL>
  g_dfused_pivots += snap.n_dfused;
  // a job of a batch that is neither primal nor dual feasible: nothing has ended, the single-handle path carries on from
  // the pivots made so far and books its own
  if (done == D_NEED_PHASE1) return 0;
  P->last_ms = last_ms;
  P->hint_dual = false;
  switch (done) {
    case D_OPT: P->status = MVX_OPT; return 0;
    case D_UNBND: P->status = MVX_UNBND; return 0;
    case D_NOFEAS: P->status = MVX_NOFEAS; return 0;
    case D_ITLIM: P->status = (snap.phase == PH_PRIMAL2) ? MVX_FEAS : MVX_INFEAS; return MVX_EITLIM;
    default: P->status = MVX_UNDEF; return MVX_EFAIL;
  }
}

// The staging buffer holds the control block and, because the solve has ended (k_export packs the
// mirrors whenever done != RUN), the basis / solution mirrors: publish them on the handle.
static bool job_finalize(SolveJob &J) {
  mvx_prob *P = J.P;
  SolveCtx &sc = *J.sc;
  publish_mirrors(P, StageView(sc.h_stage, P->m_cap, P->ld));
  float ms = 0.f;
  HIPCHECK(hipEventElapsedTime(&ms, sc.ev_a, sc.ev_b));
  J.rc = book_result(P, J.snap, J.done, ms);
  return true;
}

// the job's stream has been synchronised; returns true when the solve is complete
static bool job_collect(Context &c, SolveJob &J) {
  SolveCtx &sc = *J.sc;
  Ctl &snap = J.snap;
  if (J.persist_queued) {
    J.persist_queued = false;
    if (sc.h_pabort[0]) {
      // the resident-tableau launch gave up waiting for its peers: its workgroups may have stopped one step apart,
      // so the tableau is put back as it was in front of the launch and the two-kernel path carries on from there
      mvx_prob *P = J.P;
      g_persist_broken = true;
      g_persist_aborts++;
      std::fprintf(stderr, "mvx: resident-tableau launch aborted (workgroups not co-resident in time); using the two-kernel path from now on\n");
      HIPCHECK(hipMemcpyAsync(P->slab, sc.p_backup, P->slab_bytes, hipMemcpyDeviceToDevice, sc.stream));
      HIPCHECK(hipMemcpyAsync(sc.d_ctl, sc.d_pctl, sizeof(Ctl), hipMemcpyDeviceToDevice, sc.stream));
      HIPCHECK(hipMemcpyAsync(sc.d_pw[0], sc.d_ppw, (size_t)P->ld * 8, hipMemcpyDeviceToDevice, sc.stream));
      HIPCHECK(hipMemcpyAsync(sc.d_pw[1], sc.d_ppw + P->ld, (size_t)P->ld * 8, hipMemcpyDeviceToDevice, sc.stream));
      HIPCHECK(hipMemsetAsync(sc.d_pabort, 0, sizeof(int), sc.stream));
      sc.h_pabort[0] = 0;
      J.try_fused = true; // the backup was taken right after a generic step in primal phase 2
      return false;
    }
  }
  std::memcpy(&snap, sc.h_stage, sizeof(Ctl));
  if (J.mode == SolveJob::FINAL) return job_finalize(J);
  if (J.mode == SolveJob::PHASE1) {
    if (snap.done == D_RUN) {
      J.pb = std::min(J.pb * 2, 64);
      return false;
    }
    if (snap.done == D_PFEAS) {
      snap.rounds++;
      if (snap.rounds >= 64) {
        J.done = D_FAIL;
        J.mode = SolveJob::FINAL;
        return false;
      }
      snap.done = D_RUN;
      snap.phase = PH_START;
      *sc.h_ctl = snap;
      upload_ctl(sc);
      J.mode = SolveJob::MAIN;
      J.batch = 8;
      J.try_fused = false;
      J.try_dfused = false;
      return false;
    }
    J.done = snap.done;
    return job_finalize(J); // the same batch's export already packed the mirrors
  }
  if (J.profiled) {
    // once the solve finishes inside a batch the queued-ahead launches are no-ops; only the
    // leading launches that really stepped are timed
    const int steps_now = snap.n_bulk; // launches that stepped: one per pivot or flip, one per chain of pivots
    flush_update_events(c, std::min(J.ev_used, (size_t)2 * (size_t)(steps_now - J.seen_steps)));
    J.seen_steps = steps_now;
  }
  if (snap.cl_abort) {
    // a cluster launch gave up waiting for its peers: it changed nothing, the rest of the batch returned at once and
    // the closing generic step carried on; from here on the chains are chosen by k_pc / k_pr
    g_cluster_broken.store(true);
    g_cluster_aborts++;
    std::fprintf(stderr, "mvx: cluster selection launch aborted (peer workgroups not reachable in time); using two launches per chained step from now on\n");
    HIPCHECK(hipMemsetAsync(sc.d_xabort, 0, sizeof(int), sc.stream));
  }
  J.done = snap.done;
  {
    // chains that keep ending early (bound flips, degenerate stretches, the end of the solve) leave their queued
    // selection launches as no-ops: follow the length the last batch actually reached
    const int dp = snap.it_cnt - J.seen_pivots, db = snap.n_bulk - J.seen_bulk;
    if (J.chain0 > 1 && db >= 4) {
      if (2 * dp < J.chain * db) J.chain = std::max(1, J.chain / 2);
      else if (10 * dp >= 9 * J.chain * db) J.chain = std::min(J.chain0, J.chain * 2);
    }
    J.seen_bulk = snap.n_bulk;
  }
  J.seen_pivots = snap.it_cnt;
  J.try_fused = (snap.phase == PH_PRIMAL2) && snap.stall < snap.stall_limit; // the fused path prices by Dantzig only
  J.try_dfused = (snap.phase == PH_DUAL) && snap.stall < snap.stall_limit && dual_fused_worth_it(J.P);
  if (J.done == D_NEED_PHASE1) {
    snap.done = D_RUN;
    snap.phase = PH_PHASE1;
    snap.p1_init = 1; // k_p1_head zeroes the cost row (tableau row m+1) and the signs
    snap.p1_fix_q = 0;
    *sc.h_ctl = snap;
    upload_ctl(sc);
    J.mode = SolveJob::PHASE1;
    J.pb = 4;
    return false;
  }
  if (J.done != D_RUN) return job_finalize(J); // the same batch's export already packed the mirrors
  J.batch = std::min(J.batch * 2, 256);
  return false;
}

// A handle whose last solve ended OPT and that has not been edited since (every edit resets `status`)
// would go through zero pivots and come out unchanged: bs.cpp:116-117 re-solves exactly such clones at
// every pop.  Answer from the state at hand instead of queueing launches.  NOFEAS / UNBND are not in the
// list: a new call restarts the devex weights, so the re-solve may pick another infeasible row (another
// entering column) than the one that proved infeasibility (unboundedness) and pivot on before it ends there again.
static bool already_solved(const mvx_prob *P, const mvx_smcp &parm) {
  if (!P->valid || parm.it_lim == 0) return false;
  if (P->status != MVX_OPT) return false;
  return P->last_tol[0] == parm.tol_bnd && P->last_tol[1] == parm.tol_dj && P->last_tol[2] == parm.tol_piv;
}
static void remember_tolerances(mvx_prob *P, const mvx_smcp &parm) {
  P->last_tol[0] = parm.tol_bnd;
  P->last_tol[1] = parm.tol_dj;
  P->last_tol[2] = parm.tol_piv;
}

// What every solve does with a handle before any device work, single or in a batch.  true: the handle goes on to the
// device, with a tableau; false: the call ends here for it with *rc.
static bool admit(mvx_prob *P, const mvx_smcp &parm, int *rc) {
  if (P->m < 1 || P->n < 1) {
    P->status = MVX_UNDEF;
    *rc = MVX_EFAIL;
    return false;
  }
  if (already_solved(P, parm)) {
    P->last_ms = 0.0;
    *rc = 0;
    return false;
  }
  if (!P->valid && !build_slack_tableau(P)) {
    *rc = MVX_EFAIL;
    return false;
  }
  remember_tolerances(P, parm);
  P->fresh_rows = -1; // the solve rewrites the tableau: whatever ends it exports the mirrors anew, or leaves them stale
  return true;
}

static bool job_prepare(SolveJob &J, mvx_prob *P, const mvx_smcp *parm) {
  J.P = P;
  if (parm) J.parm = *parm;
  else mvx_init_smcp(&J.parm);
  return admit(P, J.parm, &J.rc);
}

static int solve_once(mvx_prob *P, const mvx_smcp *parm, bool aux) {
  SolveJob J;
  if (!job_prepare(J, P, parm)) return J.rc;
  Context &c = ctx();
  HIPCHECK(hipSetDevice(c.dev)); // the current device is per host thread (the B&B driver solves from a worker thread)
  std::unique_lock<std::recursive_mutex> main_lock(c.main_mu);
  flush_copies(c);
  if (aux) main_lock.unlock();
  std::unique_lock<std::mutex> aux_lock(c.aux_mu, std::defer_lock);
  if (aux) aux_lock.lock();
  if (aux && !c.aux_ready) {
    init_solve_ctx(c.aux);
    c.aux_ready = true;
  }
  J.sc = aux ? &c.aux : &c.main;
  static std::atomic<bool> g_resident_token{false};
  bool expected = false;
  J.resident = g_resident_token.compare_exchange_strong(expected, true);
  job_begin(c, J);
  for (;;) {
    job_enqueue(c, J);
    HIPCHECK(hipStreamSynchronize(J.sc->stream));
    if (job_collect(c, J)) break;
  }
  if (J.resident) g_resident_token.store(false);
  return J.rc;
}

// ---- tableau refresh (same rule and arithmetic as the oracle's refresh_tableau / orc_row_residual)
static int g_check_every = 1024;
static double g_refresh_tol = 1e-9;
void set_refresh(int check_every, double tol) {
  g_check_every = check_every > 0 ? check_every : 1024;
  g_refresh_tol = tol >= 0.0 ? tol : 1e-9;
}

constexpr int REFRESH_SAMPLE_ROWS = 32; // rows the look that decides on a refresh reads (oracle: REFRESH_SAMPLE_ROWS)
static double row_residual_sample(const mvx_prob *P, int rows);
double row_residual(const mvx_prob *P) { return row_residual_sample(P, 0); }

// residual over `rows` rows picked from the pivot count (rows <= 0 or >= m: every row)
static double row_residual_sample(const mvx_prob *P, int rows) {
  if (!P->valid) return 0.0;
  refresh_solution(P);
  const int m = P->m, n = P->n;
  auto value = [&](int k) {
    const int pos = P->pos[(size_t)k];
    if (pos > 0) return P->beta[(size_t)pos];
    double lb, ub;
    var_bounds(P, k, &lb, &ub);
    return nb_value(P->nflag[(size_t)-pos], lb, ub);
  };
  std::vector<double> x((size_t)n + 1, 0.0);
  for (int j = 1; j <= n; j++) x[(size_t)j] = value(m + j);
  double worst = 0.0;
  const bool all = rows <= 0 || rows >= m;
  const int cnt = all ? m : rows;
  for (int k = 0; k < cnt; k++) {
    const int i = all ? k + 1 : 1 + (int)(((unsigned)P->it_cnt * 2654435761u + (unsigned)k * 0x9E3779B1u) % (unsigned)m);
    const double *a = P->A[(size_t)i]->data();
    double acc = 0.0;
    for (int j = 1; j <= n; j++) acc = acc + a[j] * x[(size_t)j];
    const double xr = value(i);
    const double r = std::fabs(acc - xr) / (1.0 + std::fabs(xr));
    if (r > worst) worst = r;
  }
  return worst;
}

static bool refresh_tableau(mvx_prob *P) {
  Context &c = ctx();
  MAIN_LOCK(c);
  flush_copies(c);
  SolveCtx &sc = c.main;
  const int m = P->m, n = P->n;
  std::vector<int> tflag((size_t)m + n + 1, 0), sflag((size_t)n + 1, 0);
  for (int j = 1; j <= n; j++) tflag[(size_t)P->nvar[(size_t)j]] = P->nflag[(size_t)j];
  for (int j = 1; j <= n; j++) sflag[(size_t)j] = tflag[(size_t)m + j] ? tflag[(size_t)m + j] : std_flag(P->ctype[(size_t)j]);
  const int status = P->status;
  if (!build_slack_tableau(P, sflag.data())) return false;
  ensure_scratch(sc, P->m_cap, P->ld);
  HIPCHECK(hipMemcpyAsync(sc.d_tflag, tflag.data(), tflag.size() * 4, hipMemcpyHostToDevice, sc.stream));
  fill_ctl(sc, P, sc.h_ctl);
  upload_ctl(sc);
  for (int k = m + 1; k <= m + n; k++) {
    if (tflag[(size_t)k]) continue; // non-basic in the target basis
    launch_refresh_select(sc.d_ctl, sc.d_tflag, k, sc.stream);
    launch_update(sc.d_ctl, m, n, sc.stream);
  }
  launch_export(sc.d_ctl, sc.d_stage, m, n, 1, sc.stream);
  pull_stage(sc, P, true); // synchronises: tflag / the control block may go out of scope
  P->status = status;
  P->refresh_cnt++;
  return true;
}

// the counter / residual / refresh step that follows every solve (oracle: orc_simplex)
// scripts/bnbrepeat.py: [0] tableau refreshes, [1] residual looks, [2] single-handle solves, [3] batch calls, [4] jobs a batch
// handed to the single-handle path (neither primal nor dual feasible)
static std::atomic<long long> g_dbg[8];
extern "C" void mvx_debug_counters(long long *out, int reset) {
  for (int k = 0; k < 8; k++) {
    out[k] = g_dbg[k].load();
    if (reset) g_dbg[k].store(0);
  }
}

// oracle: NOFEAS_RECHECK / largest_violation -- a NOFEAS verdict whose largest violation is within the rounding an
// ill-conditioned tableau puts on column 0 counts on a rebuilt tableau only.  A recheck, not a cure: column 0 still drifts
// on such a basis.  (The oracle's refresh_tableau cannot fail; here a rebuild that cannot get its slab leaves the verdict
// as it is.)  A verdict above the threshold is not looked at again here; mvx_farkas_many (engine_farkas_many below, DESIGN.md
// "Infeasibility and unboundedness proofs (farkas)") asks the model, not the tableau, whether any MVX_NOFEAS verdict holds.
constexpr double NOFEAS_RECHECK = 1e-6;
static double largest_violation(const mvx_prob *P) {
  refresh_solution(P);
  double worst = 0.0;
  for (int i = 1; i <= P->m; i++) {
    double lb, ub, v = 0.0;
    var_bounds(P, P->bvar[(size_t)i], &lb, &ub);
    const double beta = P->beta[(size_t)i];
    if (lb > -INFINITY && beta < lb) v = (lb - beta) / (1.0 + std::fabs(lb));
    if (ub < INFINITY && beta > ub) v = (beta - ub) / (1.0 + std::fabs(ub));
    if (v > worst) worst = v;
  }
  return worst;
}

static int after_solve(mvx_prob *P, const mvx_smcp *parm, int rc, int pivots) {
  P->piv_since_check += pivots;
  if (rc == 0 && P->status == MVX_NOFEAS && P->it_cnt > 0 && largest_violation(P) <= NOFEAS_RECHECK && refresh_tableau(P)) {
    g_dbg[0]++;
    P->piv_since_check = 0;
    const int before = P->it_cnt;
    P->status = MVX_UNDEF;
    rc = solve_once(P, parm, true); // the pivot limit of the call, if any, applies to this leg afresh
    P->piv_since_check += P->it_cnt - before;
  }
  if (rc == 0 && P->status == MVX_OPT && P->piv_since_check >= g_check_every) {
    P->piv_since_check = 0;
    g_dbg[1]++;
    if (row_residual_sample(P, REFRESH_SAMPLE_ROWS) > g_refresh_tol && refresh_tableau(P)) {
      g_dbg[0]++;
      const int before = P->it_cnt;
      // the rebuilt tableau has not been looked at by anything yet: the simplex runs on it whatever the status says (the
      // oracle's simplex_once has no "already solved" shortcut) -- it may be infeasible or non-optimal beyond the
      // tolerance, or a numerically singular column may have been skipped
      P->status = MVX_UNDEF;
      rc = solve_once(P, parm, true); // the pivot limit of the call, if any, applies to this leg afresh
      P->piv_since_check += P->it_cnt - before;
    }
  }
  return rc;
}

static int engine_simplex_on(mvx_prob *P, const mvx_smcp *parm, bool aux) {
  const int before = P->it_cnt;
  g_dbg[2]++;
  const int rc = solve_once(P, parm, aux);
  return after_solve(P, parm, rc, P->it_cnt - before);
}

int engine_simplex(mvx_prob *P, const mvx_smcp *parm) { return engine_simplex_on(P, parm, false); }

// ------------------------------------------------------------------------ batched solves
// Independent node LPs (the two children of a branch, a window of open B&B nodes) advance together:
// ONE launch of k_select / k_update carries every slot of the batch (grid.z = slot), each slot
// with its own control block and scratch.  Small tableaux are bound by the dispatch rate of tiny
// kernels (measured: 8 streams give only ~1.7x), so the slots share launches instead of competing
// for them.  The handles form a work queue on the device: the host uploads one control block per handle
// and the slots pull them (k_select: a slot whose solve has ended exports its mirrors into the job's
// staging area and takes the next job in the very launch that finds it idle), so slots do not sit
// idle until the host's next synchronisation point -- the host only polls two counters.  Results are
// bit-identical to one mvx_simplex call per handle: every job runs the same generic state machine
// (k_select) on its own data.
struct BatchCtx {
  int slots = 0, jobs = 0;
  int m_cap = 0, ld = 0; // per-slot scratch capacity
  hipStream_t stream = nullptr;
  Ctl *d_ctl = nullptr, *h_ctl = nullptr;   // slot control blocks (host copy: the idle pattern)
  Ctl *d_jobs = nullptr, *h_jobs = nullptr; // job control blocks
  Ctl *h_fill = nullptr;                    // slot control blocks read back for the tail compaction
  hipEvent_t poll_ev = nullptr;             // follows each poll's copies on `stream`
  SlotScratch *d_sp = nullptr, *h_sp = nullptr;
  int *d_cnt = nullptr, *h_cnt = nullptr; // [0] next job, [1] finished jobs, [2] rounds launched, [3] round of the last job's end
  int pred_rounds = 16;                   // rounds the previous batch on this context needed
  unsigned char *scratch = nullptr;
  size_t scratch_stride = 0;
  unsigned char *d_stage = nullptr, *h_stage = nullptr; // one staging area per JOB
  size_t stage_stride = 0;
};
// Two batch contexts (stream, slot control blocks, scratch, staging): two host threads can each drive a batched solve
// at the same time -- the B&B driver splits a round's children over two workers, so that the host side of one batch
// (uploads, polls, result mirrors) overlaps the kernels of the other.
constexpr int N_BATCH_CTX = 8;
static BatchCtx g_batch[N_BATCH_CTX];
static std::mutex g_batch_mu[N_BATCH_CTX];
static void sync_batch_stream() {
  for (int k = 0; k < N_BATCH_CTX; k++)
    if (g_batch[k].stream) HIPCHECK(hipStreamSynchronize(g_batch[k].stream));
}
static int g_batch_slots = 64;

// a device / pinned host array of `count` elements in place of the one p holds, if any; nothing is kept
template <class T>
static void renew_dev(T *&p, size_t count) {
  if (p) HIPCHECK(hipFree(p));
  HIPCHECK(hipMalloc((void **)&p, sizeof(T) * count));
}
template <class T>
static void renew_host(T *&p, size_t count) {
  if (p) HIPCHECK(hipHostFree(p));
  HIPCHECK(hipHostMalloc((void **)&p, sizeof(T) * count));
}

// every piece of one slot's scratch, in layout order (see Pieces); returns a slot's bytes
static size_t slot_pieces(SlotScratch &sp, int mc, int l, unsigned char *base) {
  const size_t row = (size_t)mc + 1, col = (size_t)l, var = (size_t)mc + l + 1;
  Pieces piece{base};
  piece(sp.colq, row), piece(sp.srow, col), piece(sp.olb, var), piece(sp.oub, var), piece(sp.dw, row);
  piece(sp.pw, col); // generic path only: one set of primal weights
  // dual chains: DCH_MAX - 1 pairs (pivot column, scaled pivot row); k_select finds their parts by the two strides
  const size_t o_chain = piece.carve.off;
  piece(sp.chain, row);
  sp.chain_col = piece.carve.off - o_chain;
  piece.carve(col * 8);
  sp.chain_stride = piece.carve.off - o_chain;
  piece.carve((size_t)(DCH_MAX - 2) * sp.chain_stride);
  return piece.carve.off;
}

static void ensure_batch(BatchCtx &bc, int slots, int jobs, int m_cap, int ld) {
  if (!bc.stream) HIPCHECK(hipStreamCreateWithFlags(&bc.stream, hipStreamNonBlocking));
  if (!bc.poll_ev) HIPCHECK(hipEventCreateWithFlags(&bc.poll_ev, hipEventDisableTiming));
  if (slots <= bc.slots && jobs <= bc.jobs && m_cap <= bc.m_cap && ld <= bc.ld) return;
  HIPCHECK(hipStreamSynchronize(bc.stream));
  bc.slots = std::max(slots, bc.slots);
  bc.jobs = std::max(jobs + jobs / 2, bc.jobs);
  bc.m_cap = std::max(m_cap, bc.m_cap);
  bc.ld = std::max(ld, bc.ld);
  SlotScratch measure;
  bc.scratch_stride = slot_pieces(measure, bc.m_cap, bc.ld, nullptr);
  bc.stage_stride = StageView::bytes(bc.m_cap, bc.ld);
  renew_dev(bc.d_ctl, bc.slots), renew_host(bc.h_ctl, bc.slots);
  renew_dev(bc.d_jobs, bc.jobs), renew_host(bc.h_jobs, bc.jobs);
  renew_host(bc.h_fill, bc.slots);
  renew_dev(bc.d_sp, bc.slots), renew_host(bc.h_sp, bc.slots);
  renew_dev(bc.d_cnt, 4), renew_host(bc.h_cnt, 8);
  renew_dev(bc.scratch, bc.scratch_stride * bc.slots);
  renew_dev(bc.d_stage, bc.stage_stride * bc.jobs), renew_host(bc.h_stage, bc.stage_stride * bc.jobs);
  HIPCHECK(hipMemsetAsync(bc.d_cnt, 0, sizeof(int) * 4, bc.stream)); // on the batch's own stream: a null-stream memset is not ordered with it
  HIPCHECK(hipMemsetAsync(bc.scratch, 0, bc.scratch_stride * bc.slots, bc.stream));
  for (int k = 0; k < bc.slots; k++) slot_pieces(bc.h_sp[k], bc.m_cap, bc.ld, bc.scratch + (size_t)k * bc.scratch_stride);
  HIPCHECK(hipMemcpyAsync(bc.d_sp, bc.h_sp, sizeof(SlotScratch) * bc.slots, hipMemcpyHostToDevice, bc.stream));
  // an idle slot reads as finished and holds no job
  std::memset(bc.h_ctl, 0, sizeof(Ctl) * bc.slots);
  for (int k = 0; k < bc.slots; k++) {
    bc.h_ctl[k].done = D_FAIL;
    bc.h_ctl[k].job = -1;
  }
}

// control block of one job; the scratch pointers, chain_max, pc_epoch and npb stay zero: the slot that pulls the job points
// it at its own scratch (k_select)
static void batch_fill_job(Ctl *h, mvx_prob *P, const mvx_smcp &parm, int njobs) {
  ctl_for_handle(h, P, parm.tol_bnd, parm.tol_dj, parm.tol_piv, pivot_budget(P, parm));
  h->job = -1;
  h->dchain_max = dual_chain_length(njobs >= 32, P->m <= 1024 && P->n <= 1024);
  take_edits(P, h);
}

// mirrors + status of a finished job; layout inside the staging area follows the handle's own m_cap / ld
static int batch_finish_job(BatchCtx &bc, int j, mvx_prob *P, int *done_code, int *pivots) {
  unsigned char *s = bc.h_stage + (size_t)j * bc.stage_stride;
  Ctl snap;
  std::memcpy(&snap, s, sizeof(Ctl));
  *done_code = snap.done;
  *pivots = snap.it_cnt;
  if (snap.done != D_NEED_PHASE1) publish_mirrors(P, StageView(s, P->m_cap, P->ld));
  return book_result(P, snap, snap.done, 0.0);
}

int engine_simplex_batch(mvx_prob **probs, int count, const mvx_smcp *parm_in, int *rcs) {
  if (count <= 0) return 0;
  Context &c = ctx();
  HIPCHECK(hipSetDevice(c.dev)); // per host thread, see engine_simplex
  mvx_smcp parm;
  if (parm_in) parm = *parm_in;
  else mvx_init_smcp(&parm);
  std::vector<int> pending, fallback;
  int m_cap = 0, ld = 0, m_max = 0, n_max = 0;
  for (int i = 0; i < count; i++) {
    mvx_prob *P = probs[i];
    int rc = 0;
    if (!admit(P, parm, &rc)) {
      if (rcs) rcs[i] = rc;
      continue;
    }
    pending.push_back(i);
    m_cap = std::max(m_cap, P->m_cap);
    ld = std::max(ld, P->ld);
    m_max = std::max(m_max, P->m);
    n_max = std::max(n_max, P->n);
  }
  {
    MAIN_LOCK(c);
    flush_copies(c); // clones recorded since the last device call: one launch for all of them
  }
  if (pending.size() == 1) { // nothing to share a launch with
    const int i = pending[0];
    HIPCHECK(hipStreamSynchronize(c.main.stream)); // edits queued on the main stream first
    const int rc = engine_simplex_on(probs[i], &parm, true);
    if (rcs) rcs[i] = rc;
    return 0;
  }
  if (pending.empty()) return 0;
  // whichever batch context is free; all busy: wait for the first
  std::unique_lock<std::mutex> batch_lock;
  int which = -1;
  for (int k = 0; k < N_BATCH_CTX && which < 0; k++) {
    batch_lock = std::unique_lock<std::mutex>(g_batch_mu[k], std::try_to_lock);
    if (batch_lock.owns_lock()) which = k;
  }
  if (which < 0) {
    batch_lock = std::unique_lock<std::mutex>(g_batch_mu[0]);
    which = 0;
  }
  BatchCtx &bc = g_batch[which];
  g_dbg[3]++;
  const int njobs = (int)pending.size();
  const int K = std::min(njobs, g_batch_slots);
  ensure_batch(bc, K, njobs, m_cap, ld);
  // edits queued on the main stream (bound changes, clones) must be visible to the batch stream
  HIPCHECK(hipStreamSynchronize(c.main.stream));
  for (int j = 0; j < njobs; j++) batch_fill_job(&bc.h_jobs[j], probs[pending[(size_t)j]], parm, njobs);
  bc.h_cnt[0] = bc.h_cnt[1] = bc.h_cnt[2] = bc.h_cnt[3] = 0;
  HIPCHECK(hipMemcpyAsync(bc.d_jobs, bc.h_jobs, sizeof(Ctl) * (size_t)njobs, hipMemcpyHostToDevice, bc.stream));
  HIPCHECK(hipMemcpyAsync(bc.d_ctl, bc.h_ctl, sizeof(Ctl) * (size_t)K, hipMemcpyHostToDevice, bc.stream)); // every slot idle
  HIPCHECK(hipMemcpyAsync(bc.d_cnt, bc.h_cnt, sizeof(int) * 4, hipMemcpyHostToDevice, bc.stream));
  BatchQueue q;
  q.jobs = bc.d_jobs;
  q.scratch = bc.d_sp;
  q.counters = bc.d_cnt;
  q.stage = bc.d_stage;
  q.stage_stride = bc.stage_stride;
  q.count = njobs;
  // Rounds queued ahead of the host.  The slots refill themselves, so a poll only has to notice the end; every round
  // queued past the end is three launches that start only to leave (~12 us), and every poll the stream waits for is a
  // host round trip with the GPU idle (~20 us).  So the polls are pipelined: burst k is queued BEFORE the host looks at
  // the poll that followed burst k-1 -- the stream never runs dry, at the price of at most one short burst of empty
  // rounds.  MVX_BATCH_FIRST / MVX_BATCH_BURST: rounds in the first / in every later burst (8 / 4; sweeps of 4..16 and
  // 2..8 are within the noise of one another).  MVX_BATCH_PRED=1 sizes the first burst by the previous batch on this
  // context (the device records the round in which the last job ended): measured no better, a poll early on lets the
  // tail shrink sooner.
  static const bool predict = std::getenv("MVX_BATCH_PRED") && std::atoi(std::getenv("MVX_BATCH_PRED")) != 0;
  static const int later = std::getenv("MVX_BATCH_BURST") ? std::max(1, std::min(64, std::atoi(std::getenv("MVX_BATCH_BURST")))) : 4;
  int Kact = K; // slots launched: all of them while the queue has work, the occupied ones once it is drained
  // slots that still hold a running solve, as of the last poll (an over-estimate by then): the update's tile depth goes
  // by the work in the launch, not by its slots -- behind the slowest LPs of a batch a launch is a few tableaux deep
  int busy = K;
  static const bool busy_tiles = !(std::getenv("MVX_BUSY_TILES") && std::atoi(std::getenv("MVX_BUSY_TILES")) == 0);
  auto launch_rounds = [&](int rounds) {
    for (int d = 0; d < rounds; d++) {
      launch_dsel(bc.d_ctl, m_max, n_max, bc.stream, Kact); // every slot whose dual phase is carrying on: its chain on chip
      launch_select_queue(bc.d_ctl, q, bc.stream, Kact);
      launch_update(bc.d_ctl, m_max, n_max, bc.stream, Kact, 1, busy_tiles ? busy : 0);
    }
  };
  bool with_fill = false; // the poll in flight carries the slots' control blocks (the queue was drained when it was queued)
  auto queue_poll = [&](bool fill) {
    HIPCHECK(hipMemcpyAsync(bc.h_cnt + 4, bc.d_cnt, sizeof(int) * 4, hipMemcpyDeviceToHost, bc.stream));
    with_fill = fill && Kact > 1;
    if (with_fill) HIPCHECK(hipMemcpyAsync(bc.h_fill, bc.d_ctl, sizeof(Ctl) * (size_t)Kact, hipMemcpyDeviceToHost, bc.stream));
    HIPCHECK(hipEventRecord(bc.poll_ev, bc.stream));
  };
  static const int first = std::getenv("MVX_BATCH_FIRST") ? std::max(1, std::min(64, std::atoi(std::getenv("MVX_BATCH_FIRST")))) : 8;
  launch_rounds(predict ? std::max(2, std::min(bc.pred_rounds, 256) - 2) : (njobs <= 2 ? std::min(8, first) : first));
  queue_poll(false);
  for (;;) {
    launch_rounds(later); // runs while the host waits for the poll queued before it
    HIPCHECK(hipEventSynchronize(bc.poll_ev));
    if (bc.h_cnt[5] >= njobs) break;
    const bool drained = bc.h_cnt[4] >= njobs; // no slot can pull a job any more
    busy = std::max(1, std::min(Kact, njobs - bc.h_cnt[5]));
    if (with_fill) {
      // Tail of the batch: the queue is empty and the slots finish one by one.  An idle slot of a launch still costs
      // its share of workgroups that start only to leave (512x1024: 132 per slot), so the control blocks that still
      // hold a job move to the front and the launches shrink.  Their pointers keep addressing their own scratch.  (The
      // snapshot is one burst old: a slot idle then is idle for good, one busy then is moved whether it has ended since
      // or not.)
      int w = 0;
      for (int k = 0; k < Kact; k++) {
        if (bc.h_fill[k].job < 0) continue;
        if (k != w) HIPCHECK(hipMemcpyAsync(&bc.d_ctl[w], &bc.d_ctl[k], sizeof(Ctl), hipMemcpyDeviceToDevice, bc.stream));
        w++;
      }
      if (w >= 1 && w < Kact) Kact = w;
    }
    queue_poll(drained);
  }
  bc.pred_rounds = std::max(1, bc.h_cnt[7]);
  HIPCHECK(hipMemcpyAsync(bc.h_stage, bc.d_stage, bc.stage_stride * (size_t)njobs, hipMemcpyDeviceToHost, bc.stream));
  HIPCHECK(hipStreamSynchronize(bc.stream));
  for (int j = 0; j < njobs; j++) {
    const int i = pending[(size_t)j];
    int code = 0, piv = 0;
    int rc = batch_finish_job(bc, j, probs[i], &code, &piv);
    if (code == D_NEED_PHASE1) {
      g_dbg[4]++;
      fallback.push_back(i);
      probs[i]->piv_since_check += piv; // the single-handle leg below adds its own and applies the refresh rule
    } else {
      rc = after_solve(probs[i], &parm, rc, piv); // residual look / tableau refresh, as after any solve
      if (rcs) rcs[i] = rc;
    }
  }
  for (int i : fallback) {
    // the batch left this handle untouched apart from zero or more completed pivots
    probs[i]->sol_fresh = false;
    probs[i]->fresh_rows = -1;
    const int rc = engine_simplex_on(probs[i], &parm, true);
    if (rcs) rcs[i] = rc;
  }
  return 0;
}

// -------------------------------------------------------------------------- model edits
// What every edit of a live tableau shares is written here once (DESIGN.md "Live edits"): the footer, the two ways of giving the
// tableau up, and the call frame of an edit with device work.
// The footer of an edit that leaves a valid tableau: what the mirrors hold of tableau rows 1..keep stays current (-1: nothing
// does), the solution is stale, the status unknown.  fresh_rows is never below -1, so keep = -1 leaves it at -1.
static void edit_footer(mvx_prob *P, int keep) {
  P->fresh_rows = P->sol_fresh ? keep : std::min(P->fresh_rows, keep);
  P->sol_fresh = false;
  P->status = MVX_UNDEF;
}
// The tableau is given up: the next solve starts from the slack basis.  release = false (the edit cannot stay warm): the slab
// is kept and the next solve builds the slack tableau in it, so a recorded clone INTO it must land first.  release = true (the
// device is out of memory): the slab goes back to the cache.
static void edit_give_up(mvx_prob *P, bool release) {
  if (release) release_device(P);
  else {
    Context &c = ctx();
    MAIN_LOCK(c);
    flush_copies(c);
  }
  engine_invalidate(P);
}
// The call frame of an edit of one handle with device work: a NodeCall that sends the recorded clones off first (a recorded
// clone of the handle receives the bits from before the edit) and brings nothing back.  The caller declares its upload pieces,
// then begin(): the reservation and, where the edit changes the slab's geometry, the move (from() / to() are the views the
// launch reads and writes, the same unless the handle moved); false sends the caller to out_of_memory().  Then the pinned side is
// filled, upload(), the launch, the mirrors, and done(keep): the old slab is recycled behind the launch, the footer, and the
// synchronise that frees the pinned block.
class LiveEdit : public NodeCall {
  mvx_prob *P_;
  SlabMove mv_;

public:
  explicit LiveEdit(mvx_prob *P) : NodeCall(NodeFlush::AtEntry, NodeResults::None), P_(P) {}
  bool begin(int m_cap, int ld) { return reserve() && slab_move(*c, P_, m_cap, ld, mv_); }
  bool begin() { return begin(P_->m_cap, P_->ld); }
  const SlabView &from() const { return mv_.from; }
  const SlabView &to() const { return mv_.to; }
  int out_of_memory() {
    edit_give_up(P_, true);
    return -2;
  }
  void done(int keep) {
    slab_move_done(*c, mv_);
    edit_footer(P_, keep);
    fetch();
  }
};
// `cnt` rows have been appended behind row m_old (P->m is the new count): the structural variable numbers move up by cnt and
// the new rows hold their own auxiliaries
static void mirrors_rows_appended(mvx_prob *P, int m_old, int cnt) {
  for (int i = 1; i <= m_old; i++)
    if (P->bvar[i] > m_old) P->bvar[i] += cnt;
  for (int q = 1; q <= P->n; q++)
    if (P->nvar[q] > m_old) P->nvar[q] += cnt;
  P->bvar.resize((size_t)P->m + 1);
  for (int t = 0; t < cnt; t++) P->bvar[(size_t)(m_old + 1 + t)] = m_old + 1 + t;
  rebuild_pos(P);
}
// What taking the indices `removed` out of 1..N does to the others, which close up in their order (tableau rows for a row
// deletion, non-basic positions for a column deletion): `first` the first removed index, src[t] the index that moves to
// first + t (ascending: what k_delrows and k_delcols are given), newpos the new index of every old one (0: removed)
struct Compaction {
  int first = 0;
  std::vector<int> src, newpos;
};
static Compaction compaction(const std::vector<int> &removed, int N) {
  Compaction pl;
  pl.newpos.assign((size_t)N + 1, 0);
  pl.first = N + 1;
  for (int i : removed) {
    pl.newpos[(size_t)i] = -1;
    pl.first = std::min(pl.first, i);
  }
  for (int i = 1, w = 0; i <= N; i++) {
    if (pl.newpos[(size_t)i]) {
      pl.newpos[(size_t)i] = 0;
      continue;
    }
    pl.newpos[(size_t)i] = ++w;
    if (i > pl.first) pl.src.push_back(i);
  }
  return pl;
}
// how many numbers of the ascending list lie below k
static int count_below(const std::vector<int> &list, int k) { return (int)(std::lower_bound(list.begin(), list.end(), k) - list.begin()); }

void engine_apply_bounds(mvx_prob *P, int k, int type, double old_lb, double old_ub, double lb, double ub) {
  if (!P->valid) return;
  Context &c = ctx();
  MAIN_LOCK(c);
  SolveCtx &sc = c.main;
  const int pos = P->pos[k];
  if (pos > 0) {
    // no launch: the edit waits on the handle and rides in the control block of the next solve (k_select applies it)
    bool merged = false;
    for (auto &e : P->pending)
      if (e.row == pos) {
        e.lb = lb;
        e.ub = ub;
        merged = true;
      }
    if (!merged) {
      if ((int)P->pending.size() == MAX_EDITS) {
        flush_copies(c); // a recorded clone INTO this handle's slab must land before the edits do
        flush_edits(sc, P);
      }
      P->pending.push_back({pos, lb, ub});
    }
    P->hint_dual = true; // a basic variable's bound moved: the warm start is a dual one (bs.cpp:274,282)
  } else {
    const int jj = -pos;
    const double xo = nb_value(P->nflag[jj], old_lb, old_ub);
    int flag;
    switch (type) {
      case MVX_FR: flag = MVX_NF; break;
      case MVX_LO: flag = MVX_NL; break;
      case MVX_UP: flag = MVX_NU; break;
      case MVX_DB: flag = (P->nflag[jj] == MVX_NU) ? MVX_NU : MVX_NL; break;
      default: flag = MVX_NS; break;
    }
    P->nflag[jj] = flag;
    flush_copies(c);
    launch_set_nonbasic(P->d_nlb, P->d_nub, P->d_nflag, jj, lb, ub, flag, sc.stream);
    const double xn = nb_value(flag, lb, ub);
    if (xn != xo) launch_shift_nonbasic(P->d_T, P->ld, P->m, jj, xn - xo, sc.stream);
  }
  edit_footer(P, -1);
}

void engine_add_rows(mvx_prob *P, int first, int nrs) {
  if (!P->valid) return;
  Context &c = ctx();
  MAIN_LOCK(c);
  SolveCtx &sc = c.main;
  flush_copies(c);
  if (!grow_rows(P, P->m)) return edit_give_up(P, true);
  launch_add_rows(P->d_T, P->ld, P->n, P->d_bvar, P->d_blb, P->d_bub, P->d_nvar, first, nrs, P->m, sc.stream);
  mirrors_rows_appended(P, first - 1, nrs); // mvx_add_rows appends: first is the old m + 1
  edit_footer(P, first - 1);                // the new rows sit behind the old ones
}

// run k_rowcomb with host-provided weights / base, writing row `dst_row` of the tableau
constexpr int RC_SLOTS = 32;
static void rowcomb_into_row(mvx_prob *P, const std::vector<double> &w, const std::vector<double> &base, int dst_row) {
  Context &c = ctx();
  MAIN_LOCK(c);
  SolveCtx &sc = c.main;
  flush_copies(c);
  ensure_scratch(sc, P->m_cap, P->ld);
  // The operands go through a pinned slot of their own, so nothing here waits for the device: a B&B round appends one
  // cut row to each of its branching nodes, and with a synchronisation in front of and behind every one of them the
  // host paid ~100 us per node for 10 us of kernels.  Whoever reads the row next does so on this stream or
  // synchronises it first (eval_tab_row, the clone launches, the batch entry).
  if (!sc.rc_ring || P->m_cap > sc.rc_m_cap || P->ld > sc.rc_ld) {
    HIPCHECK(hipStreamSynchronize(sc.stream));
    if (sc.rc_ring) HIPCHECK(hipHostFree(sc.rc_ring));
    sc.rc_m_cap = std::max(P->m_cap, sc.rc_m_cap);
    sc.rc_ld = std::max(P->ld, sc.rc_ld);
    sc.rc_slot_bytes = align_up(sizeof(Ctl), 256) + align_up((size_t)(sc.rc_m_cap + 1) * 8, 256) + align_up((size_t)sc.rc_ld * 8, 256);
    HIPCHECK(hipHostMalloc((void **)&sc.rc_ring, sc.rc_slot_bytes * RC_SLOTS));
    sc.rc_next = 0;
  }
  if (sc.rc_next == RC_SLOTS) { // every slot may still be in flight
    HIPCHECK(hipStreamSynchronize(sc.stream));
    sc.rc_next = 0;
  }
  unsigned char *slot = sc.rc_ring + sc.rc_slot_bytes * (size_t)sc.rc_next++;
  Ctl *hc = (Ctl *)slot;
  double *hw = (double *)(slot + align_up(sizeof(Ctl), 256));
  double *hb = (double *)((unsigned char *)hw + align_up((size_t)(sc.rc_m_cap + 1) * 8, 256));
  fill_ctl(sc, P, hc);
  hc->rc_base = sc.d_rcbase;
  hc->rc_out = P->d_T + (size_t)dst_row * P->ld;
  std::memcpy(hw, w.data(), (size_t)(P->m + 1) * 8);
  std::memcpy(hb, base.data(), (size_t)(P->n + 1) * 8);
  HIPCHECK(hipMemcpyAsync(sc.d_ctl, hc, sizeof(Ctl), hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipMemcpyAsync(sc.d_wts, hw, (size_t)(P->m + 1) * 8, hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipMemcpyAsync(sc.d_rcbase, hb, (size_t)(P->n + 1) * 8, hipMemcpyHostToDevice, sc.stream));
  launch_rowcomb(sc.d_ctl, P->m, P->n, 0, sc.stream);
}

void engine_row_from_model(mvx_prob *P, int i) {
  // x_i = sum_j v_j x_(m+j): substitute the basic structurals by their tableau rows
  const int m = P->m, n = P->n;
  const int pos = P->pos[i];
  const double *a = P->A[i]->data();
  std::vector<double> w((size_t)m + 1, 0.0), base((size_t)n + 1, 0.0);
  for (int r = 1; r <= m; r++)
    if (r != pos && P->bvar[r] > m) w[r] = a[P->bvar[r] - m];
  double b0 = 0.0;
  for (int jj = 1; jj <= n; jj++) {
    if (P->nvar[jj] > m) {
      const int col = P->nvar[jj] - m;
      const double v = a[col];
      const double x = nb_value(P->nflag[jj], P->clb[col], P->cub[col]);
      base[jj] = v;
      if (x != 0.0 && v != 0.0) b0 = std::fma(v, x, b0);
    }
  }
  base[0] = b0;
  rowcomb_into_row(P, w, base, pos);
  P->hint_dual = true; // appended cut rows (cut.cpp:40) leave the basis dual feasible
  edit_footer(P, pos - 1); // only tableau row `pos` has been rewritten
}

// ------------------------------------------------------------------ a round of cuts: scores (k_cutgram), append (k_cutrows)
// dot[t] = sum_j v_tj x_j and gram[t][s] = sum_j v_tj v_sj of `k` candidate rows (mvx_cut_scores; vals is k x (n+1) in the
// layout of mvx_gmi_cuts, x[1..n] the column values of the solved handle, read by the caller out of the mirrors): one upload,
// one k_cutgram launch, one copy back.  Nothing of the handle changes.  Return codes: 0; -1 bad arguments or a handle that
// is not MVX_OPT; -2 device out of memory.
int engine_cut_scores(const mvx_prob *P, int k, const double *vals, const double *x, double *dot, double *gram) {
  if (!P || k < 1 || !vals || !x || !dot || !gram || !P->valid || P->status != MVX_OPT) return -1;
  const int n = P->n;
  const size_t row = (size_t)n + 1;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  const size_t o_vals = f.up((size_t)k * row * 8), o_x = f.up(row * 8);
  const size_t o_dot = f.out((size_t)k * 8), o_gram = f.out((size_t)k * (size_t)k * 8);
  if (!f.reserve()) return -2;
  std::memcpy(f.hb + o_vals, vals, (size_t)k * row * 8);
  std::memcpy(f.hb + o_x, x, row * 8);
  *(double *)(f.hb + o_x) = 0.0; // entry 0 is not a column
  f.upload();
  CutGramArgs a;
  a.vals = (const double *)(f.db + o_vals);
  a.x = (const double *)(f.db + o_x);
  a.dot = (double *)(f.db + o_dot);
  a.gram = (double *)(f.db + o_gram);
  a.k = k; a.n = n;
  launch_cutgram(a, f.stream());
  f.fetch();
  std::memcpy(dot, f.hb + o_dot, (size_t)k * 8);
  std::memcpy(gram, f.hb + o_gram, (size_t)k * (size_t)k * 8);
  return 0;
}

// `k` dense MVX_LO rows appended in one device pass (mvx_add_cut_rows): the handle is left as k times (add_rows(1), set_mat_row
// with all n indices, set_row_bnds(LO)) leave it -- model, mirrors, tableau, pending bound edits, fresh_rows, hint_dual,
// status -- with one grow_rows call, one renumbering of the mirrors, one upload and one k_cutrows launch (a LiveEdit).  What the kernel
// needs of the basis goes up as two index lists (the structural column of every row and of every non-basic position, taken
// before the renumbering); the weights and the base of engine_row_from_model are entries of `vals` under those lists, and
// only the row's value at the non-basic point (base[0]) is computed here, in engine_row_from_model's order.
// The bound of a new row is a pending edit, as engine_apply_bounds leaves it; of the edits that the k single calls would have
// flushed on the way (MAX_EDITS), those of new rows are written by the kernel itself and those of older rows are launched.
// Return codes: 0; -1 bad arguments, nothing changed (k < 1, a null, a NaN, a handle without a valid tableau); -2 device out of
// memory: the model has the rows and the tableau is given up.
// The host work of one handle's append, shared by engine_add_cut_rows and engine_add_cut_rows_many: the checks, the model
// rows, the pieces of the upload and what goes into them, and the ending.
// the rows that are read hold no NaN (entry 0 of a row is not read)
static bool cut_rows_readable(int n, int k, const double *vals, const double *rhs) {
  const size_t row = (size_t)n + 1;
  for (int t = 0; t < k; t++) {
    if (std::isnan(rhs[t])) return false;
    for (int j = 1; j <= n; j++)
      if (std::isnan(vals[(size_t)t * row + (size_t)j])) return false;
  }
  return true;
}
// the model: what add_rows + set_mat_row + set_row_bnds write
static void cut_rows_model(mvx_prob *P, int k, const double *vals, const double *rhs) {
  const size_t row = (size_t)P->n + 1;
  for (int t = 0; t < k; t++) {
    auto r = std::make_shared<std::vector<double>>(vals + (size_t)t * row, vals + (size_t)(t + 1) * row);
    (*r)[0] = 0.0;
    P->A.push_back(std::move(r));
    P->rtype.push_back(MVX_LO);
    P->rlb.push_back(rhs[t]);
    P->rub.push_back(INFINITY);
  }
  P->m += k;
  P->status = MVX_UNDEF;
}
// where one handle's pieces lie in the frame's arena (m: rows before the append)
struct CutRowsPieces {
  size_t o_vals, o_rowcol, o_nbcol, o_rowlb, o_extra;
};
static CutRowsPieces cut_rows_pieces(NodeCall &f, int m, int n, int k) {
  CutRowsPieces p;
  p.o_vals = f.up((size_t)k * ((size_t)n + 1) * 8), p.o_rowcol = f.up((size_t)(m + 1) * 4), p.o_nbcol = f.up(((size_t)n + 1) * 4);
  p.o_rowlb = f.up((size_t)k * 8), p.o_extra = f.up((size_t)k * 4);
  return p;
}
// fills the pinned side of the pieces from the handle as it stands before the renumbering (P->m is already m + k), and books
// the new rows' bounds as pending edits; edits of older rows that overflow on the way are launched on the frame's stream
static void cut_rows_fill(mvx_prob *P, int m, int k, const double *vals, const double *rhs, unsigned char *hb, const CutRowsPieces &p,
                          hipStream_t st) {
  const int n = P->n;
  const size_t row = (size_t)n + 1;
  double *h_vals = (double *)(hb + p.o_vals), *h_rowlb = (double *)(hb + p.o_rowlb);
  int *h_rowcol = (int *)(hb + p.o_rowcol), *h_nbcol = (int *)(hb + p.o_nbcol), *h_extra = (int *)(hb + p.o_extra);
  std::memcpy(h_vals, vals, (size_t)k * row * 8);
  h_rowcol[0] = 0;
  for (int i = 1; i <= m; i++) h_rowcol[i] = P->bvar[i] > m ? P->bvar[i] - m : 0;
  h_nbcol[0] = 0;
  for (int q = 1; q <= n; q++) h_nbcol[q] = P->nvar[q] > m ? P->nvar[q] - m : 0;
  const int real_chunks = (m + ROWCOMB_CHUNK - 1) / ROWCOMB_CHUNK;
  for (int t = 0; t < k; t++) {
    const double *a = vals + (size_t)t * row;
    double b0 = 0.0;
    for (int q = 1; q <= n; q++) {
      const int col = h_nbcol[q];
      if (!col) continue;
      const double v = a[col], x = nb_value(P->nflag[q], P->clb[col], P->cub[col]);
      if (x != 0.0 && v != 0.0) b0 = std::fma(v, x, b0);
    }
    h_vals[(size_t)t * row] = b0;
    h_extra[t] = (m + t + 1 + ROWCOMB_CHUNK - 1) / ROWCOMB_CHUNK > real_chunks ? 1 : 0;
    h_rowlb[t] = -INFINITY;
  }
  // the bounds: k set_row_bnds calls on basic rows, MAX_EDITS pending at a time
  for (int t = 0; t < k; t++) {
    if ((int)P->pending.size() == MAX_EDITS) {
      for (const auto &e : P->pending) {
        if (e.row <= m) launch_set_basic_bounds(P->d_blb, P->d_bub, e.row, e.lb, e.ub, st);
        else h_rowlb[e.row - m - 1] = e.lb;
      }
      P->pending.clear();
    }
    P->pending.push_back({m + 1 + t, rhs[t], INFINITY});
  }
}
static CutRowsArgs cut_rows_args(const SlabView &v, int m, int n, int k, const unsigned char *db, const CutRowsPieces &p) {
  CutRowsArgs a;
  a.v = v;
  a.vals = (const double *)(db + p.o_vals);
  a.rowcol = (const int *)(db + p.o_rowcol);
  a.nbcol = (const int *)(db + p.o_nbcol);
  a.rowlb = (const double *)(db + p.o_rowlb);
  a.extra = (const int *)(db + p.o_extra);
  a.m = m; a.n = n; a.k = k;
  return a;
}
// the launch is queued: the mirrors follow it, once (what remains is the footer with keep = m)
static void cut_rows_appended(mvx_prob *P, int m, int k) {
  mirrors_rows_appended(P, m, k);
  P->hint_dual = true;
}

int engine_add_cut_rows(mvx_prob *P, int k, const double *vals, const double *rhs) {
  if (!P || k < 1 || !vals || !rhs || !P->valid) return -1;
  const int m = P->m, n = P->n;
  if (!cut_rows_readable(n, k, vals, rhs)) return -1;
  cut_rows_model(P, k, vals, rhs);
  LiveEdit f(P);
  const CutRowsPieces p = cut_rows_pieces(f, m, n, k);
  if (!grow_rows(P, P->m) || !f.begin()) return f.out_of_memory();
  cut_rows_fill(P, m, k, vals, rhs, f.hb, p, f.stream());
  f.upload();
  launch_cutrows(cut_rows_args(f.to(), m, n, k, f.db, p), f.stream());
  cut_rows_appended(P, m, k);
  f.done(m);
  return 0;
}

// engine_add_cut_rows on `count` handles of the same column count in one call (mvx_add_cut_rows_many; DESIGN.md "Row append
// across handles (add_cut_rows_many)"): handle t takes rows off[t] .. off[t+1]-1 of vals / rhs, and every handle that is given
// rows ends as engine_add_cut_rows leaves it, bit for bit, through the same functions.  The device work of all of them is the
// recorded clones flushed once, one upload of [descriptors | first tiles | each handle's lists and rows] and one
// k_cutrows_many launch, with the grow_rows copies of handles that run out of spare rows and the overflowing bound edits of
// older rows queued on the same stream in front of it.  A handle that is given no rows is not touched.  Everything is checked
// before the first handle is edited.  When the arena cannot be reserved for all handles they go in two halves, and so on down to
// a single handle; that one, or one whose larger slab cannot be had, ends as engine_add_cut_rows' out-of-memory path leaves
// it while the others complete.  The frame is a NodeCall of its own: one reservation and one upload serve all handles.
// Return codes: 0; -1 bad arguments, nothing changed (a null, count < 1, a handle twice, differing column counts, a descending
// off, a NaN that would be read, a handle without a valid tableau that is given rows); -2 device out of memory for some handle.
int engine_add_cut_rows_many(mvx_prob *const *Ps, int count, const int *off, const double *vals, const double *rhs) {
  if (!Ps || count < 1 || !off || !vals || !rhs || off[0] != 0) return -1;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || off[t + 1] < off[t] || Ps[t]->n != Ps[0]->n) return -1;
  {
    std::vector<const mvx_prob *> seen(Ps, Ps + count);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return -1;
  }
  const int n = Ps[0]->n;
  const size_t row = (size_t)n + 1;
  struct Item {
    mvx_prob *P;
    const double *vals, *rhs;
    int m, k; // m: rows before the append
    CutRowsPieces p;
  };
  std::vector<Item> items;
  for (int t = 0; t < count; t++) {
    const int k = off[t + 1] - off[t];
    if (k == 0) continue; // not touched at all
    const double *v = vals + (size_t)off[t] * row, *r = rhs + off[t];
    if (!Ps[t]->valid || !cut_rows_readable(n, k, v, r)) return -1;
    items.push_back(Item{Ps[t], v, r, Ps[t]->m, k, CutRowsPieces()});
  }
  if (items.empty()) return 0;
  for (const Item &it : items) cut_rows_model(it.P, it.k, it.vals, it.rhs);
  int rc = 0;
  const size_t GRID_Y = 65535;
  // handles [lo, hi) in as few launches as the arena allows
  std::function<void(size_t, size_t)> run = [&](size_t lo, size_t hi) {
    if (hi <= lo) return;
    NodeCall f(NodeFlush::AtEntry, NodeResults::None);
    const size_t o_hs = f.up((hi - lo) * sizeof(CutRowsHandle)), o_tiles = f.up((hi - lo) * 4);
    for (size_t i = lo; i < hi; i++) items[i].p = cut_rows_pieces(f, items[i].m, n, items[i].k);
    if (!f.reserve()) {
      rc = -2;
      if (hi - lo == 1) return edit_give_up(items[lo].P, true);
      const size_t mid = lo + (hi - lo) / 2;
      run(lo, mid);
      run(mid, hi);
      return;
    }
    CutRowsHandle *hs = (CutRowsHandle *)(f.hb + o_hs);
    int *tiles = (int *)(f.hb + o_tiles);
    std::vector<Item *> done;
    size_t ntiles = 0;
    for (size_t i = lo; i < hi; i++) {
      Item &it = items[i];
      if (!grow_rows(it.P, it.P->m)) { // the model has the rows, the tableau is given up; the others complete
        edit_give_up(it.P, true);
        rc = -2;
        continue;
      }
      cut_rows_fill(it.P, it.m, it.k, it.vals, it.rhs, f.hb, it.p, f.stream());
      const CutRowsPieces &p = it.p;
      tiles[done.size()] = (int)ntiles;
      hs[done.size()] = CutRowsHandle{slab_view(it.P), p.o_vals, p.o_rowcol, p.o_nbcol, p.o_rowlb, p.o_extra, it.m, it.k, (int)ntiles, 0};
      ntiles += (size_t)(it.k + CUT_TILE - 1) / CUT_TILE;
      done.push_back(&it);
    }
    if (!done.empty()) {
      f.upload();
      for (size_t t0 = 0; t0 < ntiles; t0 += GRID_Y)
        launch_cutrows_many((const CutRowsHandle *)(f.db + o_hs), (const int *)(f.db + o_tiles), (int)done.size(), f.db, n, (int)t0,
                            (int)std::min(GRID_Y, ntiles - t0), f.stream());
      for (Item *it : done) {
        cut_rows_appended(it->P, it->m, it->k);
        edit_footer(it->P, it->m);
      }
    }
    f.fetch(); // the pinned block is free again
  };
  run(0, items.size());
  return rc;
}

// ------------------------------------------------------------------ column append and pricing (k_addcols)
// k_addcols reads the columns a tile at a time: [tile][model row][ADDCOLS_CT], zero behind column k (AddColsArgs::cols)
static size_t addcols_tiled_bytes(int k, int m) { return (size_t)((k + ADDCOLS_CT - 1) / ADDCOLS_CT) * ((size_t)m + 1) * ADDCOLS_CT * 8; }
static void addcols_tile_columns(double *dst, const double *cols, int k, int m) {
  const size_t crow = (size_t)m + 1;
  std::memset(dst, 0, addcols_tiled_bytes(k, m));
  for (int t = 0; t < k; t++) {
    double *d = dst + (size_t)(t / ADDCOLS_CT) * crow * ADDCOLS_CT + (size_t)(t % ADDCOLS_CT);
    const double *s = cols + (size_t)t * crow;
    for (size_t i = 1; i < crow; i++) d[i * ADDCOLS_CT] = s[i];
  }
}
// `k` structural columns have joined the model as columns n_old+1 .. P->n (mvx_add_dense_cols; DESIGN.md "Column append
// (add_cols)"): one upload and one k_addcols launch (a LiveEdit) make them non-basic columns of the live tableau.  cols is
// k x (m+1) by model row, flag / lb / ub the new positions' statuses and normalised bounds.  With a pool S (mvx_pool_append) the
// columns are its columns idx[0..k): cols is not read, and k_poolgather lays the tiles out on the device.  While ld_for(n) does
// not change the columns are written in place; otherwise the handle moves to a slab (m_cap, ld_for(n)) that the same launch
// writes whole.
// Pending bound edits stay pending: they are keyed by tableau row.
// Return codes: 0; -2 device out of memory, the tableau is given up.
int engine_add_cols_live(mvx_prob *P, int k, const double *cols, const double *obj, const int *flag, const double *lb, const double *ub,
                         const mvx_colpool *S, const int *idx) {
  const int m = P->m, n = P->n - k; // n: the columns of the tableau as it stands
  const size_t crow = (size_t)m + 1;
  LiveEdit f(P);
  // from a pool the tiles are not uploaded: k_poolgather writes them into a device-only piece from the pool's device copy
  const size_t o_cols = S ? 0 : f.up(addcols_tiled_bytes(k, m)), o_obj = f.up((size_t)k * 8), o_xs = f.up((size_t)k * 8);
  const size_t o_lb = f.up((size_t)k * 8), o_ub = f.up((size_t)k * 8), o_flag = f.up((size_t)k * 4);
  const size_t o_idx = S ? f.up((size_t)k * 4) : 0, o_tiles = S ? f.dev(addcols_tiled_bytes(k, m)) : o_cols;
  if ((S && engine_pool_sync(S) != 0) || !f.begin(P->m_cap, ld_for(n + k))) return f.out_of_memory();
  unsigned char *hb = f.hb, *db = f.db;
  if (S) std::memcpy(hb + o_idx, idx, (size_t)k * 4);
  else addcols_tile_columns((double *)(hb + o_cols), cols, k, m);
  std::memcpy(hb + o_obj, obj, (size_t)k * 8);
  std::memcpy(hb + o_lb, lb, (size_t)k * 8);
  std::memcpy(hb + o_ub, ub, (size_t)k * 8);
  std::memcpy(hb + o_flag, flag, (size_t)k * 4);
  double *h_xs = (double *)(hb + o_xs);
  for (int t = 0; t < k; t++) h_xs[t] = nb_value(flag[t], lb[t], ub[t]);
  f.upload();
  if (S) launch_pool_gather(PoolGatherArgs{S->d_cols, (const int *)(db + o_idx), (double *)(db + o_tiles), m, S->h.ldp, k}, f.stream());
  AddColsArgs a;
  std::memset(&a, 0, sizeof a);
  a.s = f.from();
  a.d = f.to();
  a.cols = (const double *)(db + o_tiles);
  a.obj = (const double *)(db + o_obj);
  a.xs = (const double *)(db + o_xs);
  a.nlb_new = (const double *)(db + o_lb);
  a.nub_new = (const double *)(db + o_ub);
  a.nflag_new = (const int *)(db + o_flag);
  a.m = m; a.n = n; a.k = k;
  a.rows = m + 1;
  a.rows_all = P->m_cap + 1;
  launch_addcols(a, f.stream());
  // host mirrors
  P->nvar.resize((size_t)n + k + 1);
  P->nflag.resize((size_t)n + k + 1);
  for (int t = 0; t < k; t++) {
    P->nvar[(size_t)(n + 1 + t)] = m + n + 1 + t;
    P->nflag[(size_t)(n + 1 + t)] = flag[t];
  }
  rebuild_pos(P);
  P->hint_dual = false;
  P->dmat.reset();
  P->rmod.reset();
  f.done(-1);
  return 0;
}

// The images k_addcols would append, without appending (mvx_price_cols): dj[t] row 0 of image t, img (nullable) k x (m+1).  Pure.
// The candidates go through the node-entry arena a range at a time; a range the arena cannot hold is halved.  Return codes: 0;
// -1 bad arguments; -2 device out of memory, nothing written; -3 no valid tableau.
int engine_price_cols(const mvx_prob *P, int k, const double *cols, const double *obj, double *dj, double *img) {
  if (!P || k < 1 || !cols || !obj || !dj) return -1;
  if (!P->valid) return -3;
  const int m = P->m, n = P->n;
  const size_t crow = (size_t)m + 1;
  std::vector<double> r_dj((size_t)k), r_img(img ? (size_t)k * crow : 0);
  int kk = k;
  for (int t0 = 0; t0 < k;) {
    const int cnt = std::min(kk, k - t0);
    NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
    const size_t o_cols = f.up(addcols_tiled_bytes(cnt, m)), o_obj = f.up((size_t)cnt * 8);
    const size_t o_dj = f.out((size_t)cnt * 8), o_img = f.out(img ? (size_t)cnt * crow * 8 : 0);
    if (!f.reserve()) {
      if (cnt == 1) return -2;
      kk = cnt / 2;
      (void)take_last_error(); // the smaller range may fit
      continue;
    }
    addcols_tile_columns((double *)(f.hb + o_cols), cols + (size_t)t0 * crow, cnt, m);
    std::memcpy(f.hb + o_obj, obj + t0, (size_t)cnt * 8);
    f.upload();
    AddColsArgs a;
    std::memset(&a, 0, sizeof a);
    a.s = slab_view(P); // no destination
    a.cols = (const double *)(f.db + o_cols);
    a.obj = (const double *)(f.db + o_obj);
    a.dj = (double *)(f.db + o_dj);
    a.img = img ? (double *)(f.db + o_img) : nullptr;
    a.m = m; a.n = n; a.k = cnt;
    a.rows = img ? m + 1 : 1;
    a.rows_all = a.rows;
    launch_addcols(a, f.stream());
    f.fetch();
    std::memcpy(r_dj.data() + t0, f.hb + o_dj, (size_t)cnt * 8);
    if (img) std::memcpy(r_img.data() + (size_t)t0 * crow, f.hb + o_img, (size_t)cnt * crow * 8);
    t0 += cnt;
  }
  std::memcpy(dj, r_dj.data(), (size_t)k * 8);
  if (img) std::memcpy(img, r_img.data(), (size_t)k * crow * 8);
  return 0;
}

// ------------------------------------------------------------------ sifting over a column pool (k_poolprice, k_poolsel_*, k_poolgather)
// The device copy of a pool (DESIGN.md "Sifting (sift)"): the host image [N][ldp], the objective and the entering statuses, in
// allocations of their own that grow by half when a later mvx_pool_add_cols outruns them (the columns already there are copied on
// the device).  0, or -2 when the device has no room: the copy it had stays as it was.
int engine_pool_sync(const mvx_colpool *S) {
  const mvx_sifting::PoolHost &h = S->h;
  if (S->dev_n == h.N) return 0;
  Context &c = ctx();
  bind_device(c);
  MAIN_LOCK(c);
  const size_t ldp = (size_t)h.ldp;
  if (h.N > S->dev_cap) {
    const int cap = (int)std::min<long long>(0x7ffffff0LL, std::max<long long>(h.N, (long long)S->dev_cap + S->dev_cap / 2));
    double *nc = nullptr, *no = nullptr;
    int *nf = nullptr;
    if (hipMalloc((void **)&nc, std::max<size_t>((size_t)cap * ldp * 8, 8)) != hipSuccess ||
        hipMalloc((void **)&no, (size_t)cap * 8) != hipSuccess || hipMalloc((void **)&nf, (size_t)cap * 4) != hipSuccess) {
      (void)hipGetLastError();
      if (nc) (void)hipFree(nc);
      if (no) (void)hipFree(no);
      g_last_error.store(MVX_ENOMEM);
      return -2;
    }
    HIPCHECK(hipStreamSynchronize(c.main.stream)); // nothing queued reads the old copy any more
    if (S->dev_n > 0) {
      if (ldp) HIPCHECK(hipMemcpy(nc, S->d_cols, (size_t)S->dev_n * ldp * 8, hipMemcpyDeviceToDevice));
      HIPCHECK(hipMemcpy(no, S->d_obj, (size_t)S->dev_n * 8, hipMemcpyDeviceToDevice));
      HIPCHECK(hipMemcpy(nf, S->d_flag, (size_t)S->dev_n * 4, hipMemcpyDeviceToDevice));
    }
    if (S->d_cols) HIPCHECK(hipFree(S->d_cols));
    if (S->d_obj) HIPCHECK(hipFree(S->d_obj));
    if (S->d_flag) HIPCHECK(hipFree(S->d_flag));
    S->d_cols = nc, S->d_obj = no, S->d_flag = nf;
    S->dev_cap = cap;
  }
  const size_t n0 = (size_t)S->dev_n, cnt = (size_t)h.N - n0;
  std::vector<int> flag(cnt);
  for (size_t t = 0; t < cnt; t++) flag[t] = std_flag(h.type[n0 + t]);
  if (ldp) HIPCHECK(hipMemcpy(S->d_cols + n0 * ldp, h.cols.data() + n0 * ldp, cnt * ldp * 8, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(S->d_obj + n0, h.obj.data() + n0, cnt * 8, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(S->d_flag + n0, flag.data(), cnt * 4, hipMemcpyHostToDevice));
  S->dev_n = h.N;
  return 0;
}
void engine_pool_release(mvx_colpool *S) {
  if (!S->d_cols && !S->d_obj && !S->d_flag) return; // the pool never met a device
  Context &c = ctx();
  bind_device(c);
  MAIN_LOCK(c);
  HIPCHECK(hipStreamSynchronize(c.main.stream));
  if (S->d_cols) HIPCHECK(hipFree(S->d_cols));
  if (S->d_obj) HIPCHECK(hipFree(S->d_obj));
  if (S->d_flag) HIPCHECK(hipFree(S->d_flag));
  S->d_cols = S->d_obj = nullptr;
  S->d_flag = nullptr;
  S->dev_n = S->dev_cap = 0;
}

// The reduced costs of every pool column against the handle's row 0 and the K most attractive of them (mvx_pool_price): one
// upload of [where the auxiliaries sit | skip], k_pooly, k_poolprice, the selection launches, one copy back of [picks | dj].
// Pure.  sgn +1 under MVX_MAX, -1 under MVX_MIN.  dj (nullable) [N+1], pick [K], *npick.  Return codes: 0; -2 device out of
// memory, nothing written; -3 no valid tableau.
int engine_pool_price(const mvx_prob *P, const mvx_colpool *S, const unsigned char *skip, int K, double sgn, double tol, double *dj, int *pick,
                      int *npick) {
  if (!P->valid) return -3;
  const int m = P->m, N = S->h.N, ldp = S->h.ldp;
  if (N == 0) {
    if (dj) dj[0] = 0.0;
    *npick = 0;
    return 0;
  }
  K = std::min(K, N);
  if (engine_pool_sync(S) != 0) return -2;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  const size_t o_ypos = f.up(((size_t)m + 1) * 4), o_skip = f.up(skip ? (size_t)N + 1 : 0);
  const size_t o_pick = f.out(((size_t)K + 1) * 4), o_dj = dj ? f.out(((size_t)N + 1) * 8) : f.dev(((size_t)N + 1) * 8);
  const size_t pick_end = o_pick + ((size_t)K + 1) * 4;
  const size_t o_y = f.dev((size_t)std::max(ldp, 1) * 8), o_key = f.dev(((size_t)N + 1) * 8), o_sel = f.dev((size_t)POOLSEL_INTS * 4);
  const size_t o_ck = f.dev((size_t)std::max(K, 1) * 8), o_cj = f.dev((size_t)std::max(K, 1) * 4);
  if (!f.reserve()) return -2;
  int *ypos = (int *)(f.hb + o_ypos);
  ypos[0] = 0;
  for (int i = 1; i <= m; i++) ypos[i] = P->pos[(size_t)i] < 0 ? -P->pos[(size_t)i] : 0;
  if (skip) std::memcpy(f.hb + o_skip, skip, (size_t)N + 1);
  f.upload();
  PoolPriceArgs a;
  std::memset(&a, 0, sizeof a);
  a.cols = S->d_cols, a.obj = S->d_obj, a.flag = S->d_flag;
  a.skip = skip ? f.db + o_skip : nullptr;
  a.T0 = P->d_T;
  a.ypos = (const int *)(f.db + o_ypos);
  a.y = (double *)(f.db + o_y);
  a.d = (double *)(f.db + o_dj);
  a.key = (unsigned long long *)(f.db + o_key);
  a.sel = (int *)(f.db + o_sel);
  a.cand_key = (unsigned long long *)(f.db + o_ck);
  a.cand_j = (int *)(f.db + o_cj);
  a.pick = (int *)(f.db + o_pick);
  a.sgn = sgn, a.tol = tol;
  a.m = m, a.ldp = ldp, a.N = N, a.K = K;
  launch_pool_price(a, f.stream());
  if (K < 1) HIPCHECK(hipMemsetAsync(f.db + o_pick, 0, 4, f.stream()));
  if (dj) HIPCHECK(hipMemsetAsync(f.db + o_dj, 0, 8, f.stream())); // dj[0]
  f.copy_back(dj ? 0 : pick_end);
  f.sync();
  const int *r = (const int *)(f.hb + o_pick);
  *npick = r[0];
  std::memcpy(pick, r + 1, (size_t)r[0] * 4);
  if (dj) std::memcpy(dj, f.hb + o_dj, ((size_t)N + 1) * 8);
  return 0;
}

// ------------------------------------------------------------------ column deletion (k_delcols)
// Model columns `cols` (ascending, distinct, numbered as before the call) have left the model (mvx_del_cols; DESIGN.md "Column
// deletion (del_cols)"; P->n is the new column count, the mirrors and P->pos still describe the n_old columns; lb / ub are the
// deleted columns' normalised bounds, in the order of `cols`).  The device copies of the model cover all columns and are dropped.
// With a valid tableau: when every deleted column is non-basic, one upload and one k_delcols launch take their positions out --
// column 0 is shifted for their resting values in ascending position order, the kept positions close up in their order bit
// for bit with nflag / nlb / nub, the structural variables are renumbered on the device and in the mirrors -- and the basis
// stays what it was (a LiveEdit).  While ld_for(n) does not change this happens in place; otherwise the handle moves to a slab
// (m_cap, ld_for(n)) that the same launch writes whole.  The rows behind row m take part: the first of them holds the cost row
// of the last primal phase 1 (tableau row m+1, see Ctl), so they are not zero over the whole stride; in place they close up
// like the others, on a relayout they are written as zeros.
// Pending bound edits stay pending: they are keyed by tableau row, and no row moves.  When a deleted column is basic it cannot
// leave without a pivot: the tableau is given up.
// Return codes: 0; -2 device out of memory, the tableau is given up.
int engine_del_cols(mvx_prob *P, const std::vector<int> &cols, int n_old, const double *lb, const double *ub) {
  P->dmat.reset();
  P->rmod.reset();
  if (!P->valid) return 0;
  const int m = P->m, ncs = (int)cols.size(), n_new = n_old - ncs;
  std::vector<int> delpos; // deleted positions
  delpos.reserve((size_t)ncs);
  for (int j : cols) {
    const int pos = P->pos[(size_t)(m + j)];
    if (pos > 0) {
      edit_give_up(P, false);
      return 0;
    }
    delpos.push_back(-pos);
  }
  std::sort(delpos.begin(), delpos.end());
  const Compaction pl = compaction(delpos, n_old); // over the non-basic positions
  const int first = pl.first, nmove = (int)pl.src.size();
  std::vector<int> sh_pos; // the deleted positions that rest on a non-zero value, ascending, and the negated values
  std::vector<double> sh_negx;
  for (int q : delpos) {
    const size_t t = (size_t)count_below(cols, P->nvar[(size_t)q] - m);
    const double x = nb_value(P->nflag[(size_t)q], lb[t], ub[t]);
    if (x != 0.0) {
      sh_pos.push_back(q);
      sh_negx.push_back(-x);
    }
  }
  const int nsh = (int)sh_pos.size();
  LiveEdit f(P);
  const size_t o_src = f.up((size_t)std::max(1, nmove) * 4), o_del = f.up((size_t)ncs * 4);
  const size_t o_shp = f.up((size_t)std::max(1, nsh) * 4), o_shx = f.up((size_t)std::max(1, nsh) * 8);
  if (!f.begin(P->m_cap, ld_for(n_new))) return f.out_of_memory();
  unsigned char *hb = f.hb, *db = f.db;
  if (nmove) std::memcpy(hb + o_src, pl.src.data(), (size_t)nmove * 4);
  std::memcpy(hb + o_del, cols.data(), (size_t)ncs * 4);
  if (nsh) {
    std::memcpy(hb + o_shp, sh_pos.data(), (size_t)nsh * 4);
    std::memcpy(hb + o_shx, sh_negx.data(), (size_t)nsh * 8);
  }
  f.upload();
  DelColsArgs a;
  std::memset(&a, 0, sizeof a);
  a.s = f.from();
  a.d = f.to();
  a.src = (const int *)(db + o_src);
  a.delc = (const int *)(db + o_del);
  a.sh_pos = (const int *)(db + o_shp);
  a.sh_negx = (const double *)(db + o_shx);
  a.m = m; a.n_old = n_old; a.ncs = ncs; a.first = first; a.nmove = nmove; a.nsh = nsh;
  a.rows_all = P->m_cap + 1;
  launch_delcols(a, f.stream());
  // host mirrors: the same compaction and renumbering
  auto renumber = [&](int k) { return k <= m ? k : k - count_below(cols, k - m); };
  for (int i = 1; i <= m; i++) P->bvar[(size_t)i] = renumber(P->bvar[(size_t)i]);
  for (int q = 1; q <= n_old; q++) {
    const size_t w = (size_t)pl.newpos[(size_t)q]; // w <= q
    if (!w) continue;
    P->nvar[w] = renumber(P->nvar[(size_t)q]);
    P->nflag[w] = P->nflag[(size_t)q];
  }
  P->nvar.resize((size_t)n_new + 1);
  P->nflag.resize((size_t)n_new + 1);
  rebuild_pos(P);
  if (nsh) P->hint_dual = true; // resting values left column 0: the reduced costs stand, a basic variable may have left its bounds
  f.done(-1);
  return 0;
}

// Model rows `rows` (ascending, distinct, numbered as before the call) have left the model (mvx_del_rows; P->m is the new row
// count, the mirrors and P->pos still describe the m_old rows).  The device copies of the model that cover one of them are
// dropped.  With a valid tableau: when every deleted row's auxiliary variable is basic, its tableau rows are taken out in place
// by one k_delrows launch -- the rows that stay keep their order and their bits, bvar / blb / bub move with them, the variable
// numbers are rewritten on the device and in the mirrors, pending edits follow their rows -- and the basis stays what it was,
// so a solve that follows takes no pivot.  The map goes up through the node entries' pinned block; nothing waits for the device
// in front of the launch.  When a deleted row's auxiliary is non-basic, the column it holds cannot be dropped without a pivot:
// the tableau is given up.
// false: a deleted row's auxiliary variable is non-basic (the plan, over tableau rows, is then not filled in)
static bool del_plan(const mvx_prob *P, const std::vector<int> &rows, int m_old, Compaction &pl) {
  std::vector<int> gone; // tableau rows
  gone.reserve(rows.size());
  for (int i : rows) {
    if (P->pos[i] <= 0) return false;
    gone.push_back(P->pos[i]);
  }
  pl = compaction(gone, m_old);
  return true;
}
// the host side of a planned deletion: the mirrors take the kernel's compaction and renumbering, pending bound edits follow
// their rows; what the mirrors hold of the rows in front of the first removed one stays current (the caller's footer)
static void del_mirrors(mvx_prob *P, const std::vector<int> &rows, int m_old, const Compaction &pl) {
  const int nrs = (int)rows.size(), n = P->n;
  auto renumber = [&](int k) { return k > m_old ? k - nrs : k - count_below(rows, k); };
  for (int r = 1; r <= m_old; r++)
    if (pl.newpos[(size_t)r]) P->bvar[(size_t)pl.newpos[(size_t)r]] = renumber(P->bvar[(size_t)r]);
  P->bvar.resize((size_t)P->m + 1);
  for (int q = 1; q <= n; q++) P->nvar[(size_t)q] = renumber(P->nvar[(size_t)q]);
  rebuild_pos(P);
  // those of removed rows have nothing left to apply to
  size_t w = 0;
  for (const auto &e : P->pending)
    if (pl.newpos[(size_t)e.row]) P->pending[w++] = {pl.newpos[(size_t)e.row], e.lb, e.ub};
  P->pending.resize(w);
}
static void del_drop_model_copies(mvx_prob *P, const std::vector<int> &rows) {
  if (P->dmat && rows.front() <= P->dmat->m0) P->dmat.reset();
  if (P->rmod && rows.front() <= P->rmod->m0) P->rmod.reset();
}

// one handle's k_delrows arguments; the two lists are already in device memory
static DelRowsArgs delrows_args(const mvx_prob *P, const Compaction &pl, int m_old, const int *d_src, int nrs, const int *d_del) {
  return DelRowsArgs{slab_view(P), d_src, d_del, pl.first, (int)pl.src.size(), m_old, nrs, P->n};
}

void engine_del_rows(mvx_prob *P, const std::vector<int> &rows, int m_old) {
  del_drop_model_copies(P, rows);
  if (!P->valid) return;
  const int nrs = (int)rows.size();
  Compaction pl;
  if (!del_plan(P, rows, m_old, pl)) return edit_give_up(P, false);
  const int nmove = (int)pl.src.size();
  LiveEdit f(P);
  const size_t o_src = f.up((size_t)std::max(1, nmove) * 4), o_del = f.up((size_t)nrs * 4);
  if (!f.begin()) {
    f.out_of_memory();
    return;
  }
  if (nmove) std::memcpy(f.hb + o_src, pl.src.data(), (size_t)nmove * 4);
  std::memcpy(f.hb + o_del, rows.data(), (size_t)nrs * 4);
  f.upload();
  launch_delrows(delrows_args(P, pl, m_old, (const int *)(f.db + o_src), nrs, (const int *)(f.db + o_del)), f.stream());
  del_mirrors(P, rows, m_old, pl); // host mirrors: the same compaction and renumbering
  f.done(pl.first - 1);
}

// engine_del_rows on `count` handles whose models have been edited (mvx_del_rows_many): handle t has lost rows[t] (ascending,
// old numbers, not empty) of its m_old[t] rows.  Every handle ends as engine_del_rows leaves it, bit for bit; the device work
// of all of them is one upload of [descriptors | src and del lists] and one k_delrows_many launch behind the recorded clones,
// with no synchronise in front.  A handle without a tableau, or with a non-basic deleted row (tableau given up), takes no part
// in the launch.  When the arena cannot be reserved for all of them the handles go in two halves, and so on down to a single
// handle, which then ends as engine_del_rows' out-of-memory path leaves it.  The frame is a NodeCall of its own: one
// reservation and one upload serve all handles, and each handle takes its ending from the same functions.
void engine_del_rows_many(mvx_prob *const *Ps, int count, const std::vector<int> *rows, const int *m_old) {
  struct Item {
    mvx_prob *P;
    const std::vector<int> *rows;
    int m_old;
    Compaction pl;
  };
  std::vector<Item> items;
  for (int t = 0; t < count; t++) {
    del_drop_model_copies(Ps[t], rows[t]);
    if (Ps[t]->valid) items.push_back(Item{Ps[t], &rows[t], m_old[t], Compaction()});
  }
  size_t w = 0;
  for (size_t k = 0; k < items.size(); k++) {
    if (!del_plan(items[k].P, *items[k].rows, items[k].m_old, items[k].pl)) {
      edit_give_up(items[k].P, false);
      continue;
    }
    if (w != k) items[w] = std::move(items[k]);
    w++;
  }
  items.resize(w);
  const size_t GRID_Y = 65535;
  // handles [lo, hi) in as few launches as the arena allows
  std::function<void(size_t, size_t)> run = [&](size_t lo, size_t hi) {
    if (hi <= lo) return;
    if (hi - lo > GRID_Y) {
      run(lo, lo + GRID_Y);
      run(lo + GRID_Y, hi);
      return;
    }
    NodeCall f(NodeFlush::AtEntry, NodeResults::None);
    size_t ints = 0; // the lists of all handles lie back to back behind the descriptors: src, then del, handle by handle
    for (size_t k = lo; k < hi; k++) ints += items[k].pl.src.size() + items[k].rows->size();
    const size_t o_hs = f.up((hi - lo) * sizeof(DelRowsArgs)), o_lists = f.up(std::max<size_t>(1, ints) * 4);
    if (!f.reserve()) {
      if (hi - lo == 1) return edit_give_up(items[lo].P, true);
      const size_t mid = lo + (hi - lo) / 2;
      run(lo, mid);
      run(mid, hi);
      return;
    }
    DelRowsArgs *hs = (DelRowsArgs *)(f.hb + o_hs);
    size_t o = o_lists;
    int max_ld = 0;
    for (size_t k = lo; k < hi; k++) {
      const Item &it = items[k];
      const mvx_prob *P = it.P;
      const size_t nmove = it.pl.src.size(), nrs = it.rows->size();
      const size_t o_src = o, o_del = o + nmove * 4;
      if (nmove) std::memcpy(f.hb + o_src, it.pl.src.data(), nmove * 4);
      std::memcpy(f.hb + o_del, it.rows->data(), nrs * 4);
      o = o_del + nrs * 4;
      hs[k - lo] = delrows_args(P, it.pl, it.m_old, (const int *)(f.db + o_src), (int)nrs, (const int *)(f.db + o_del));
      max_ld = std::max(max_ld, P->ld);
    }
    f.upload();
    launch_delrows_many((const DelRowsArgs *)(f.db + o_hs), (int)(hi - lo), max_ld, f.stream());
    for (size_t k = lo; k < hi; k++) {
      del_mirrors(items[k].P, *items[k].rows, items[k].m_old, items[k].pl);
      edit_footer(items[k].P, items[k].pl.first - 1);
    }
    f.fetch(); // the pinned block is free again
  };
  run(0, items.size());
}

void engine_recompute_cost_row(mvx_prob *P) {
  if (!P->valid) return;
  const int m = P->m, n = P->n;
  std::vector<double> w((size_t)m + 1, 0.0), base((size_t)n + 1, 0.0);
  for (int i = 1; i <= m; i++) w[i] = (P->bvar[i] > m) ? P->c[P->bvar[i] - m] : 0.0;
  double z = P->c[0];
  for (int j = 1; j <= n; j++) {
    const int k = P->nvar[j];
    const double cj = (k > m) ? P->c[k - m] : 0.0;
    double lb, ub;
    var_bounds(P, k, &lb, &ub);
    const double x = nb_value(P->nflag[j], lb, ub);
    base[j] = cj;
    if (x != 0.0 && cj != 0.0) z = std::fma(cj, x, z);
  }
  base[0] = z;
  rowcomb_into_row(P, w, base, 0);
  edit_footer(P, -1);
}

void engine_invalidate(mvx_prob *P) {
  P->pending.clear();
  P->valid = false;
  P->sol_fresh = false;
  P->fresh_rows = -1;
  P->status = MVX_UNDEF;
}

void engine_copy(mvx_prob *dst, const mvx_prob *src) {
  // host fields were copied by the caller; clone the slab device-to-device
  dst->slab = nullptr;
  dst->slab_bytes = 0;
  dst->d_T = nullptr;
  if (!src->valid) {
    dst->valid = false;
    return;
  }
  Context &c = ctx();
  bind_device(c);
  MAIN_LOCK(c);
  SolveCtx &sc = c.main;
  void *slab = slab_alloc(c, src->slab_bytes);
  if (!slab) { // out of memory: the clone keeps the model only (mvx_last_error() reads MVX_ENOMEM)
    dst->valid = false;
    dst->sol_fresh = false;
    dst->fresh_rows = -1;
    dst->status = MVX_UNDEF;
    return;
  }
  bind_slab(dst, slab, src->m_cap, src->ld);
  // only the live rows of T need to travel; the small arrays follow T in one contiguous tail.  When the
  // spare rows in between are few (B&B clones of a small tableau) one range over the whole slab is cheaper
  // than two
  SlabLayout L = slab_layout(src->m_cap, src->ld);
  const size_t live = (size_t)(src->m + 1) * src->ld * 8;
  const bool whole = L.o_bvar - live <= (size_t)1 << 20;
  if (L.total <= ((size_t)64 << 20)) {
    // small tableau: record the clone; it leaves with the others of this round in one k_copy_many launch.  A source
    // that is itself waiting to be written by a recorded clone goes first.
    const unsigned char *lo = (const unsigned char *)src->slab, *hi = lo + src->slab_bytes;
    for (const CopyJob &j : c.copies)
      if ((const unsigned char *)j.dst >= lo && (const unsigned char *)j.dst < hi) {
        flush_copies(c);
        break;
      }
    if (whole) {
      c.copies.push_back({src->slab, slab, L.total});
    } else {
      c.copies.push_back({src->d_T, dst->d_T, live});
      c.copies.push_back({(const unsigned char *)src->slab + L.o_bvar, (unsigned char *)slab + L.o_bvar, L.total - L.o_bvar});
    }
    if (c.copies.size() >= 4 * COPY_BATCH) flush_copies(c);
  } else if (whole) {
    HIPCHECK(hipMemcpyAsync(slab, src->slab, L.total, hipMemcpyDeviceToDevice, sc.stream));
  } else {
    HIPCHECK(hipMemcpyAsync(dst->d_T, src->d_T, live, hipMemcpyDeviceToDevice, sc.stream));
    HIPCHECK(hipMemcpyAsync((unsigned char *)slab + L.o_bvar, (const unsigned char *)src->slab + L.o_bvar, L.total - L.o_bvar,
                            hipMemcpyDeviceToDevice, sc.stream));
  }
  dst->valid = true;
}

int engine_get_tableau(const mvx_prob *P, double *out) {
  if (!P->valid) return -1;
  Context &c = ctx();
  MAIN_LOCK(c);
  SolveCtx &sc = c.main;
  flush_copies(c);
  HIPCHECK(hipMemcpy2DAsync(out, (size_t)(P->n + 1) * 8, P->d_T, (size_t)P->ld * 8, (size_t)(P->n + 1) * 8, (size_t)P->m + 1,
                            hipMemcpyDeviceToHost, sc.stream));
  HIPCHECK(hipStreamSynchronize(sc.stream));
  return 0;
}

int engine_get_row(const mvx_prob *P, int row, double *out) {
  if (!P->valid) return -1;
  Context &c = ctx();
  MAIN_LOCK(c);
  SolveCtx &sc = c.main;
  flush_copies(c);
  HIPCHECK(hipMemcpyAsync(out, P->d_T + (size_t)row * P->ld, (size_t)(P->n + 1) * 8, hipMemcpyDeviceToHost, sc.stream));
  HIPCHECK(hipStreamSynchronize(sc.stream));
  return 0;
}

// ------------------------------------------------------------------------ GMI cuts (gmi.cpp:11-117)
static std::shared_ptr<DevMatrix> build_dev_matrix(Context &c, const mvx_prob *P, int rows = -1) { // rows: only the first `rows` (default: all)
  SolveCtx &sc = c.main;
  auto D = std::make_shared<DevMatrix>();
  const int m0 = (rows >= 0 && rows < P->m) ? rows : P->m, n = P->n;
  const int lda = (int)align_up((size_t)n + 1, LD_ALIGN);
  D->m0 = m0;
  D->n = n;
  D->lda = lda;
  std::vector<double> plain((size_t)(m0 + 1) * lda, 0.0), packed;
  std::vector<int> len((size_t)m0 + 1, 0);
  bool dense = true;
  for (int i = 1; i <= m0; i++) {
    const double *a = P->A[(size_t)i]->data();
    D->rows.push_back(P->A[(size_t)i]);
    std::memcpy(&plain[(size_t)i * lda + 1], a + 1, (size_t)n * 8);
    int l = 0;
    for (int j = 1; j <= n; j++) l += (a[j] != 0.0);
    len[(size_t)i] = l;
    dense = dense && l == n;
  }
  const size_t bytes = plain.size() * 8;
  if (hipMalloc((void **)&D->plain, bytes) != hipSuccess) {
    (void)hipGetLastError();
    g_last_error.store(MVX_ENOMEM);
    D->plain = nullptr;
    return nullptr;
  }
  HIPCHECK(hipMemcpyAsync(D->plain, plain.data(), bytes, hipMemcpyHostToDevice, sc.stream));
  if (dense) {
    D->packed = D->plain;
  } else {
    packed.assign(plain.size(), 0.0);
    for (int i = 1; i <= m0; i++) {
      const double *a = P->A[(size_t)i]->data();
      int l = 0;
      for (int j = 1; j <= n; j++)
        if (a[j] != 0.0) packed[(size_t)i * lda + (size_t)(++l)] = a[j];
    }
    if (hipMalloc((void **)&D->packed, bytes) != hipSuccess || hipMalloc((void **)&D->len, len.size() * 4) != hipSuccess) {
      (void)hipGetLastError();
      g_last_error.store(MVX_ENOMEM);
      return nullptr;
    }
    HIPCHECK(hipMemcpyAsync(D->packed, packed.data(), bytes, hipMemcpyHostToDevice, sc.stream));
    HIPCHECK(hipMemcpyAsync(D->len, len.data(), len.size() * 4, hipMemcpyHostToDevice, sc.stream));
  }
  HIPCHECK(hipStreamSynchronize(sc.stream)); // the pageable sources above go out of scope
  return D;
}

// the handle's device matrix still describes its first m0 model rows?
static bool dev_matrix_current(const mvx_prob *P) {
  const DevMatrix *D = P->dmat.get();
  if (!D || D->n != P->n || D->m0 > P->m) return false;
  for (int i = 1; i <= D->m0; i++)
    if (D->rows[(size_t)i - 1] != P->A[(size_t)i]) return false;
  return true;
}

// `count` cuts, cut t taken from the solved handle Ps[t] for its structural column cols[t] (1-based, basic):
// vals[t][0..n] with vals[t][0] = rhs[t] = the cut's lower bound (gmi.cpp:91-109), ok[t] = 0 where no valid cut exists.
// mode 0 = generateCut3 as written (gmi.cpp:11-117), 1 = the repaired formula (mvx_generateCutGMI).  The handles share
// their columns and their first m0 model rows (B&B nodes of one tree: the root's rows are the same objects in every
// clone); each has its own tableau, basis and appended cut rows.  One launch pair for all of them: a round of a B&B
// window takes one cut from each of its branching nodes (bs.cpp:249-258 with cut.cpp:20's "last cut only").
static int gmi_core(mvx_prob *const *Ps, int mode, const int *cols, int count, double *vals, double *rhs, int *ok) {
  if (count < 1) return -1;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  const int n = Ps[0]->n;
  int mmax = 0;
  for (int t = 0; t < count; t++) {
    if (!Ps[t]->valid || Ps[t]->n != n) return -1;
    mmax = std::max(mmax, Ps[t]->m);
  }
  // One device copy of the model rows the handles have in common serves them all: the rows every handle shares, object
  // for object, from row 1 on (the root's rows, and the cut rows of the ancestors the whole window descends from); what
  // a handle has beyond that -- its own lineage's cut rows -- is added on the host below, as for rows appended later.
  int common = Ps[0]->m;
  for (int t = 1; t < count; t++) {
    const mvx_prob *P = Ps[t];
    common = std::min(common, P->m);
    int i = 1;
    while (i <= common && P->A[(size_t)i].get() == Ps[0]->A[(size_t)i].get()) i++;
    common = i - 1;
  }
  if (common < 1) return -3; // not clones of one root
  std::shared_ptr<DevMatrix> Dp;
  for (int t = 0; t < count; t++) { // the deepest copy at hand that covers no more than the common rows
    const mvx_prob *P = Ps[t];
    if (P->dmat && P->dmat->m0 <= common && dev_matrix_current(P) && (!Dp || P->dmat->m0 > Dp->m0)) Dp = P->dmat;
  }
  if (!Dp) {
    Dp = build_dev_matrix(*f.c, Ps[0], common);
    if (!Dp) return -2;
  }
  for (int t = 0; t < count; t++) Ps[t]->dmat = Dp; // (their children inherit it)
  const DevMatrix &D = *Dp;
  const size_t wld = align_up((size_t)mmax + n + 1, 32), old = align_up((size_t)n + 1, 32);
  // [node descriptors x count][kind i32 x (n+1)] go up; [rhs][ok][out][work] come back (work: the auxiliaries' part only)
  const size_t o_nodes = f.up((size_t)count * sizeof(GmiNode)), o_kind = f.up((size_t)(n + 1) * 4);
  const size_t o_rhs = f.out((size_t)count * 8), o_ok = f.out((size_t)count * 4);
  const size_t o_out = f.out((size_t)count * old * 8), o_work = f.out((size_t)count * wld * 8);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  GmiNode *h_nodes = (GmiNode *)(hb + o_nodes);
  int *h_kind = (int *)(hb + o_kind);
  bool own_rows = false;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    const int j = cols[t];
    if (j < 1 || j > n || P->pos[(size_t)P->m + j] <= 0) return -1; // the column must be basic (gmi.cpp:23)
    h_nodes[t] = GmiNode{node_ref(P), P->pos[(size_t)P->m + j], 0};
    own_rows = own_rows || P->m > D.m0;
  }
  h_kind[0] = 0;
  for (int j = 1; j <= n; j++) h_kind[j] = Ps[0]->kind[(size_t)j];
  f.upload();
  GmiArgs a;
  a.nodes = (const GmiNode *)(db + o_nodes);
  a.kind = (const int *)(db + o_kind);
  a.work = (double *)(db + o_work); a.rhs = (double *)(db + o_rhs); a.ok = (int *)(db + o_ok);
  a.A = mode == 0 ? D.packed : D.plain; a.len = mode == 0 ? D.len : nullptr; a.out = (double *)(db + o_out);
  a.n = n; a.wld = (int)wld; a.lda = D.lda; a.m0 = D.m0; a.old = (int)old; a.count = count; a.mode = mode;
  launch_gmi(a, f.stream());
  f.copy_back(o_work); // rhs, ok, out
  if (own_rows) // the auxiliaries of the rows appended since: their terms are added below
    HIPCHECK(hipMemcpy2DAsync(hb + o_work, wld * 8, db + o_work, wld * 8, (size_t)(mmax + 1) * 8, (size_t)count, hipMemcpyDeviceToHost, f.stream()));
  f.sync();
  const double *h_rhs = (const double *)(hb + o_rhs), *h_out = (const double *)(hb + o_out), *h_work = (const double *)(hb + o_work);
  const int *h_ok = (const int *)(hb + o_ok);
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    double *v = vals + (size_t)t * (n + 1);
    std::memcpy(v + 1, h_out + (size_t)t * old + 1, (size_t)n * 8);
    // rows m0+1..m (this node's own cut rows) in order, the way gmi.cpp:81-89 / the repaired loop continue
    for (int i = D.m0 + 1; i <= P->m; i++) {
      const double wi = h_work[(size_t)t * wld + i];
      const double *ai = P->A[(size_t)i]->data();
      if (mode == 0) {
        int l = 0;
        for (int j = 1; j <= n; j++)
          if (ai[j] != 0.0) {
            ++l;
            v[l] += wi * ai[j]; // position l, not column j (gmi.cpp:87)
          }
      } else {
        if (wi == 0.0) continue;
        for (int j = 1; j <= n; j++)
          if (ai[j] != 0.0) v[j] += wi * ai[j];
      }
    }
    v[0] = h_rhs[t];
    rhs[t] = h_rhs[t];
    ok[t] = h_ok[t];
  }
  return 0;
}

int engine_gmi_cuts(const mvx_prob *Pc, int mode, const int *cols, int count, double *vals, double *rhs, int *ok) {
  if (count < 1) return -1;
  std::vector<mvx_prob *> Ps((size_t)count, const_cast<mvx_prob *>(Pc));
  return gmi_core(Ps.data(), mode, cols, count, vals, rhs, ok);
}

int engine_gmi_cuts_many(const mvx_prob *const *Ps, int mode, const int *cols, int count, double *vals, double *rhs, int *ok) {
  return gmi_core(const_cast<mvx_prob *const *>(Ps), mode, cols, count, vals, rhs, ok);
}

// ------------------------------------------------------------------ classification (printInfo on the device)
// The B&B drivers classify every node they pop: status, and the integer columns whose value is fractional (util.cpp:414-473).
// On the host that reads n values out of the handle's mirrors (~15 us a node on 512 x 1024, and an export first when they
// are stale).  k_classify does it for a whole batch of handles in one launch: the same selection of values the mirrors make
// (basic value from column 0 of the tableau, bound of a non-basic variable by its status -- no arithmetic, same bits), the
// same tests, and only the violated columns come back.
int engine_classify_many(const mvx_prob *const *Ps, int count, int quirks, int *status, int *nviol, int *viol, double *xviol, int cap) {
  if (count < 1 || !Ps || !status || !nviol || !viol || !xviol || cap < 1) return -1;
  for (int t = 0; t < count; t++)
    if (!Ps[t]) return -1;
  const mvx_prob *P0 = Ps[0];
  const int n = P0->n;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    if (!P->valid || P->n != n || (P != P0 && (P->c != P0->c || P->kind != P0->kind))) return -1;
  }
  NodeCall f(NodeFlush::AtEntry, NodeResults::Pinned);
  // up: [descriptors][c][kind]; out: [status][nviol][viol][xviol]; device only: [x scratch]
  const size_t o_nodes = f.up((size_t)count * sizeof(ClsNode)), o_c = f.up((size_t)(n + 1) * 8), o_kind = f.up((size_t)(n + 1) * 4);
  const size_t o_st = f.out((size_t)count * 4), o_nv = f.out((size_t)count * 4), o_viol = f.out((size_t)count * cap * 4),
               o_xv = f.out((size_t)count * cap * 8);
  const size_t o_x = f.dev((size_t)count * (n + 1) * 8);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db, *ob = f.ob;
  ClsNode *h_nodes = (ClsNode *)(hb + o_nodes);
  for (int t = 0; t < count; t++) h_nodes[t] = ClsNode{node_ref(Ps[t]), Ps[t]->status, 0};
  std::memcpy(hb + o_c, P0->c.data(), (size_t)(n + 1) * 8);
  std::memcpy(hb + o_kind, P0->kind.data(), (size_t)(n + 1) * 4);
  f.upload();
  ClsArgs a;
  a.nodes = (const ClsNode *)(db + o_nodes);
  a.c = (const double *)(db + o_c);
  a.kind = (const int *)(db + o_kind);
  a.x = (double *)(db + o_x);
  a.st = (int *)(ob + o_st); a.nv = (int *)(ob + o_nv); a.viol = (int *)(ob + o_viol); a.xv = (double *)(ob + o_xv);
  a.n = n; a.cap = cap; a.quirks = quirks; a.count = count;
  launch_classify(a, f.stream());
  f.fetch();
  const int *h_st = (const int *)(hb + o_st), *h_nv = (const int *)(hb + o_nv), *h_viol = (const int *)(hb + o_viol);
  const double *h_xv = (const double *)(hb + o_xv);
  int rc = 0;
  for (int t = 0; t < count; t++) {
    status[t] = h_st[t];
    nviol[t] = h_nv[t];
    if (h_nv[t] > cap) rc = -3;
    const int k = std::min(h_nv[t], cap);
    std::memcpy(viol + (size_t)t * cap, h_viol + (size_t)t * cap, (size_t)k * 4);
    std::memcpy(xviol + (size_t)t * cap, h_xv + (size_t)t * cap, (size_t)k * 8);
  }
  return rc;
}

// ------------------------------------------------------------------ branching penalties (k_penalty)
// One-step dual penalties of the candidate columns of a batch of solved handles (mvx_branch_penalties_many): the host finds
// each candidate's tableau row in the handle's basis mirror, one launch evaluates every (handle, candidate) pair on the
// tableaux where they lie.  Return codes: 0; -1 bad arguments or a column outside 1..n; -2 device out of memory; -3 a
// handle whose status is not MVX_OPT (or that has no tableau); -4 a column that is not basic.
int engine_penalties_many(const mvx_prob *const *Ps, int count, const int *cols, const int *col_off, double tol, double *pen_down,
                          double *pen_up, int *arg_down, int *arg_up) {
  if (count < 1 || !Ps || !cols || !col_off || !pen_down || !pen_up || !arg_down || !arg_up || col_off[0] < 0) return -1;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || col_off[t + 1] < col_off[t]) return -1;
  const int k0 = col_off[0], total = col_off[count] - k0;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    for (int k = col_off[t]; k < col_off[t + 1]; k++)
      if (cols[k] < 1 || cols[k] > P->n) return -1;
    if (!P->valid || P->status != MVX_OPT) return -3;
    for (int k = col_off[t]; k < col_off[t + 1]; k++) {
      const int row = P->pos[(size_t)(P->m + cols[k])];
      if (row < 1 || row > P->m || P->bvar[(size_t)row] != P->m + cols[k]) return -4;
    }
  }
  if (total == 0) return 0;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Pinned);
  // up: [descriptors]; out: [pen_down][pen_up][arg_down][arg_up]
  const size_t o_nodes = f.up((size_t)total * sizeof(PenNode));
  const size_t o_pd = f.out((size_t)total * 8), o_pu = f.out((size_t)total * 8), o_ad = f.out((size_t)total * 4),
               o_au = f.out((size_t)total * 4);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db, *ob = f.ob;
  PenNode *h_nodes = (PenNode *)(hb + o_nodes);
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    for (int k = col_off[t]; k < col_off[t + 1]; k++) h_nodes[k - k0] = PenNode{node_ref(P), P->pos[(size_t)(P->m + cols[k])], P->n};
  }
  f.upload();
  PenArgs a;
  a.nodes = (const PenNode *)(db + o_nodes);
  a.pen_down = (double *)(ob + o_pd); a.pen_up = (double *)(ob + o_pu);
  a.arg_down = (int *)(ob + o_ad); a.arg_up = (int *)(ob + o_au);
  a.tol = tol; a.count = total; a.pad = 0;
  launch_penalty(a, f.stream());
  f.fetch();
  std::memcpy(pen_down + k0, hb + o_pd, (size_t)total * 8);
  std::memcpy(pen_up + k0, hb + o_pu, (size_t)total * 8);
  std::memcpy(arg_down + k0, hb + o_ad, (size_t)total * 4);
  std::memcpy(arg_up + k0, hb + o_au, (size_t)total * 4);
  return 0;
}

// ------------------------------------------------------------------ sensitivity ranges (k_rangecols, k_rangefin, k_rangerows)
// Post-optimal ranges of one solved handle (mvx_ranges): nothing goes up but the kernels' arguments, which travel by value;
// three launches read the tableau, the basis and the bounds where they lie in the slab, one copy brings both tables back.
// The handle is only read.  Return codes: 0; -1 a null argument; -2 device out of memory (nothing written); -3 a handle whose
// status is not MVX_OPT or that has no tableau.
int engine_ranges(const mvx_prob *P, double tol, double *val, int *var) {
  if (!P || !val || !var) return -1;
  if (!P->valid || P->status != MVX_OPT || P->m < 1 || P->n < 1) return -3;
  const int m = P->m, n = P->n;
  const size_t rows = (size_t)m + (size_t)n + 1;
  const int nchunks = (m + RANGE_CHUNK - 1) / RANGE_CHUNK;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  // back: [val][var]; device only: [partial minima][their rows]
  const size_t o_val = f.out(rows * 6 * 8), o_var = f.out(rows * 4 * 4);
  const size_t o_pt = f.dev((size_t)2 * nchunks * (size_t)(n + 1) * 8), o_pi = f.dev((size_t)2 * nchunks * (size_t)(n + 1) * 4);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  RangeArgs a;
  a.nd = node_ref(P);
  a.blb = P->d_blb; a.bub = P->d_bub;
  a.pt = (double *)(db + o_pt); a.pi = (int *)(db + o_pi);
  a.val = (double *)(db + o_val); a.var = (int *)(db + o_var);
  a.tol = tol; a.n = n; a.nchunks = nchunks; a.maxdir = P->dir == MVX_MAX ? 1 : 0; a.pad = 0;
  launch_ranges(a, f.stream());
  f.fetch();
  std::memcpy(val, hb + o_val, rows * 6 * 8);
  std::memcpy(var, hb + o_var, rows * 4 * 4);
  std::memset(val, 0, 6 * 8); // row 0: no variable
  std::memset(var, 0, 4 * 4);
  return 0;
}

// ------------------------------------------------------------------ reduced-cost tightening (k_rcfix)
// Reduced-cost bound tightening of `count` solved handles (mvx_rc_tighten_many): one upload of the descriptors and the
// kinds, one k_rcfix launch, one copy back; the per-position results are mapped to columns through the nvar mirror and
// sorted by column.  Return codes: 0; -1 bad arguments (other column counts or kinds); -2 device out of memory; -3 a handle
// whose status is not MVX_OPT.
int engine_rc_tighten_many(const mvx_prob *const *Ps, int count, const double *cutoff, double tol, int *cnt, int *cols, double *lb,
                           double *ub) {
  if (count < 1 || !Ps || !cutoff || !cnt || !cols || !lb || !ub || !Ps[0]) return -1;
  const mvx_prob *P0 = Ps[0];
  const int n = P0->n;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    if (!P || P->n != n || (P != P0 && P->kind != P0->kind)) return -1;
  }
  for (int t = 0; t < count; t++)
    if (!Ps[t]->valid || Ps[t]->status != MVX_OPT) return -3;
  std::vector<double> z((size_t)count);
  for (int t = 0; t < count; t++) z[(size_t)t] = mvx_get_obj_val(Ps[t]); // the mirror; exports first when it is stale
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  // up: [descriptors][kind]; back: [code][val]
  const size_t o_nodes = f.up((size_t)count * sizeof(RcNode)), o_kind = f.up((size_t)(n + 1) * 4);
  const size_t o_code = f.out((size_t)count * (size_t)(n + 1) * 4), o_val = f.out((size_t)count * (size_t)(n + 1) * 8);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  RcNode *h_nodes = (RcNode *)(hb + o_nodes);
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    const double sg = P->dir == MVX_MIN ? -1.0 : 1.0, B = cutoff[t];
    const double gap = sg * z[(size_t)t] - sg * B;
    h_nodes[t] = RcNode{node_ref(P), gap + 1e-9 * std::max(1.0, std::fabs(B))};
  }
  std::memcpy(hb + o_kind, P0->kind.data(), (size_t)(n + 1) * 4);
  f.upload();
  RcArgs a;
  a.nodes = (const RcNode *)(db + o_nodes);
  a.kind = (const int *)(db + o_kind);
  a.code = (int *)(db + o_code);
  a.val = (double *)(db + o_val);
  a.tol = tol; a.n = n; a.count = count;
  launch_rcfix(a, f.stream());
  f.fetch();
  const int *h_code = (const int *)(hb + o_code);
  const double *h_val = (const double *)(hb + o_val);
  std::vector<std::pair<int, int>> hit; // (column, position)
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    const int *cd = h_code + (size_t)t * (size_t)(n + 1);
    const double *vl = h_val + (size_t)t * (size_t)(n + 1);
    hit.clear();
    for (int q = 1; q <= n; q++)
      if (cd[q] != 0) hit.emplace_back(P->nvar[(size_t)q] - P->m, q);
    std::sort(hit.begin(), hit.end());
    cnt[t] = (int)hit.size();
    for (size_t k = 0; k < hit.size(); k++) {
      const int j = hit[k].first, q = hit[k].second;
      const size_t o = (size_t)t * (size_t)n + k;
      cols[o] = j;
      lb[o] = cd[q] == 2 ? vl[q] : P->clb[(size_t)j];
      ub[o] = cd[q] == 1 ? vl[q] : P->cub[(size_t)j];
    }
  }
  return 0;
}

// ------------------------------------------------------------------ rounding heuristic (k_round)
// The model k_round reads, built from `root` and kept with it (root->rmod) for as long as rows 1..m0 are the same objects
// and the objective, kinds, direction and bounds are unchanged -- once per B&B tree.  Rows go up by column (At[j][i]) so
// that a wave reads one column of consecutive rows at a time; the locks are taken from the same rows.
static bool round_model_current(const mvx_prob *R) {
  const RoundModel *M = R->rmod.get();
  if (!M || M->m0 != R->m || M->n != R->n || M->dir != R->dir) return false;
  for (int i = 1; i <= R->m; i++)
    if (M->rows[(size_t)i - 1] != R->A[(size_t)i]) return false;
  return M->c == R->c && M->kind == R->kind && M->clb == R->clb && M->cub == R->cub && M->rlb == R->rlb && M->rub == R->rub;
}

static const RoundModel *round_model(Context &c, const mvx_prob *R) {
  if (round_model_current(R)) return R->rmod.get();
  R->rmod.reset();
  SolveCtx &sc = c.main;
  auto M = std::make_shared<RoundModel>();
  const int m0 = R->m, n = R->n;
  const size_t ldm = align_up((size_t)std::max(1, m0), 64);
  M->m0 = m0; M->n = n; M->ldm = (int)ldm; M->dir = R->dir;
  Carver carve;
  carve((size_t)(n + 1) * ldm * 8);
  M->o_rlo = carve((size_t)m0 * 8); M->o_rhi = carve((size_t)m0 * 8);
  M->o_clo = carve((size_t)(n + 1) * 8); M->o_chi = carve((size_t)(n + 1) * 8); M->o_c = carve((size_t)(n + 1) * 8);
  M->o_flags = carve((size_t)(n + 1) * 4);
  M->o_dl = carve((size_t)(n + 1) * 4); M->o_ul = carve((size_t)(n + 1) * 4); M->o_len = carve((size_t)(n + 1) * 4);
  std::vector<unsigned char> h(carve.off, 0);
  double *At = (double *)h.data();
  int *flags = (int *)(h.data() + M->o_flags);
  int *dl = (int *)(h.data() + M->o_dl), *ul = (int *)(h.data() + M->o_ul), *len = (int *)(h.data() + M->o_len);
  for (int j = 1; j <= n; j++) flags[j] = R->kind[(size_t)j] != MVX_CV ? RND_INT : 0;
  for (int i = 1; i <= m0; i++) {
    const double *ai = R->A[(size_t)i]->data();
    M->rows.push_back(R->A[(size_t)i]);
    const bool lo = std::isfinite(R->rlb[(size_t)i]), up = std::isfinite(R->rub[(size_t)i]);
    ((double *)(h.data() + M->o_rlo))[i - 1] = R->rlb[(size_t)i];
    ((double *)(h.data() + M->o_rhi))[i - 1] = R->rub[(size_t)i];
    for (int j = 1; j <= n; j++) {
      const double v = ai[j];
      At[(size_t)j * ldm + (size_t)(i - 1)] = v;
      if ((v > 0.0 && lo) || (v < 0.0 && up)) {
        flags[j] |= RND_DLOCK; // lowering x_j can break the row
        dl[j]++;
      }
      if ((v > 0.0 && up) || (v < 0.0 && lo)) {
        flags[j] |= RND_ULOCK;
        ul[j]++;
      }
      if (v != 0.0) len[j]++;
    }
  }
  std::memcpy(h.data() + M->o_clo, R->clb.data(), (size_t)(n + 1) * 8);
  std::memcpy(h.data() + M->o_chi, R->cub.data(), (size_t)(n + 1) * 8);
  std::memcpy(h.data() + M->o_c, R->c.data(), (size_t)(n + 1) * 8);
  if (hipMalloc(&M->dev, carve.off) != hipSuccess) {
    (void)hipGetLastError();
    M->dev = nullptr;
    g_last_error.store(MVX_ENOMEM);
    return nullptr;
  }
  HIPCHECK(hipMemcpyAsync(M->dev, h.data(), carve.off, hipMemcpyHostToDevice, sc.stream));
  HIPCHECK(hipStreamSynchronize(sc.stream)); // the pageable source goes out of scope
  M->c = R->c; M->kind = R->kind; M->clb = R->clb; M->cub = R->cub; M->rlb = R->rlb; M->rub = R->rub;
  R->rmod = M;
  return M.get();
}

// Primal rounding heuristic on `count` solved handles against root's model (mvx_round_many): one upload of the
// descriptors, one k_round launch, results straight into the pinned buffer.  Return codes: 0; -1 bad arguments; -2 device
// out of memory; -3 a handle whose status is not MVX_OPT; -5 n > RND_NMAX.
int engine_round_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int mode, double *obj, int *found, double *x) {
  if (!root || count < 1 || !Ps || mode < 1 || mode > 2 || !obj || !found || !x) return -1;
  const int n = root->n, m0 = root->m;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || Ps[t]->n != n) return -1;
  if (n > RND_NMAX) return -5;
  for (int t = 0; t < count; t++)
    if (!Ps[t]->valid || Ps[t]->status != MVX_OPT) return -3;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Pinned);
  const RoundModel *M = round_model(*f.c, root);
  if (!M) return -2;
  // up: [descriptors]; out: [obj][found][x]; device only: [row scratch] when the rows do not fit in LDS
  const size_t o_nodes = f.up((size_t)count * sizeof(RndNode));
  const size_t o_obj = f.out((size_t)count * 8), o_found = f.out((size_t)count * 4), o_x = f.out((size_t)count * (n + 1) * 8);
  const size_t o_scr = f.dev(m0 > RND_NMAX ? (size_t)count * m0 * 8 : 0);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db, *ob = f.ob;
  RndNode *h_nodes = (RndNode *)(hb + o_nodes);
  for (int t = 0; t < count; t++) h_nodes[t] = node_ref(Ps[t]);
  f.upload();
  const unsigned char *mb = (const unsigned char *)M->dev;
  RndArgs a;
  a.nodes = (const RndNode *)(db + o_nodes);
  a.At = (const double *)mb;
  a.rlo = (const double *)(mb + M->o_rlo); a.rhi = (const double *)(mb + M->o_rhi);
  a.clo = (const double *)(mb + M->o_clo); a.chi = (const double *)(mb + M->o_chi); a.c = (const double *)(mb + M->o_c);
  a.flags = (const int *)(mb + M->o_flags);
  a.scratch = m0 > RND_NMAX ? (double *)(db + o_scr) : nullptr;
  a.obj = (double *)(ob + o_obj); a.found = (int *)(ob + o_found); a.x = (double *)(ob + o_x);
  a.sg = root->dir == MVX_MIN ? -1.0 : 1.0;
  a.n = n; a.m0 = m0; a.ldm = M->ldm; a.mode = mode; a.count = count; a.pad = 0;
  launch_round(a, f.stream());
  f.fetch();
  std::memcpy(obj, hb + o_obj, (size_t)count * 8);
  std::memcpy(found, hb + o_found, (size_t)count * 4);
  std::memcpy(x, hb + o_x, (size_t)count * (n + 1) * 8);
  return 0;
}

// ------------------------------------------------------------------ diving pick (k_divepick)
// The branching pick of `count` (solved handle, rule) pairs against root's model (mvx_dive_pick_many): one upload of the
// descriptors, one k_divepick launch, results straight into the pinned buffer.  Return codes: 0; -1 bad arguments (a rule
// outside {1, 2, 4}, another column count); -2 device out of memory; -3 a handle whose status is not MVX_OPT; -5 n > RND_NMAX,
// as for engine_round_many, whose model it shares.
int engine_dive_pick_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, const int *rules, int *nfrac, int *col, int *dir,
                          double *val) {
  if (!root || count < 1 || !Ps || !rules || !nfrac || !col || !dir || !val) return -1;
  const int n = root->n;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || Ps[t]->n != n || (rules[t] != 1 && rules[t] != 2 && rules[t] != 4)) return -1;
  if (n > RND_NMAX) return -5;
  for (int t = 0; t < count; t++)
    if (!Ps[t]->valid || Ps[t]->status != MVX_OPT) return -3;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Pinned);
  const RoundModel *M = round_model(*f.c, root);
  if (!M) return -2;
  // up: [descriptors]; out: [nfrac][col][dir][val]
  const size_t o_nodes = f.up((size_t)count * sizeof(DiveNode));
  const size_t o_nf = f.out((size_t)count * 4), o_col = f.out((size_t)count * 4), o_dir = f.out((size_t)count * 4),
               o_val = f.out((size_t)count * 8);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db, *ob = f.ob;
  DiveNode *h_nodes = (DiveNode *)(hb + o_nodes);
  for (int t = 0; t < count; t++) h_nodes[t] = DiveNode{node_ref(Ps[t]), rules[t], 0};
  f.upload();
  const unsigned char *mb = (const unsigned char *)M->dev;
  DiveArgs a;
  a.nodes = (const DiveNode *)(db + o_nodes);
  a.c = (const double *)(mb + M->o_c);
  a.flags = (const int *)(mb + M->o_flags);
  a.dl = (const int *)(mb + M->o_dl); a.ul = (const int *)(mb + M->o_ul); a.len = (const int *)(mb + M->o_len);
  a.nfrac = (int *)(ob + o_nf); a.col = (int *)(ob + o_col); a.dir = (int *)(ob + o_dir); a.val = (double *)(ob + o_val);
  a.sg = root->dir == MVX_MIN ? -1.0 : 1.0;
  a.n = n; a.count = count;
  launch_divepick(a, f.stream());
  f.fetch();
  std::memcpy(nfrac, hb + o_nf, (size_t)count * 4);
  std::memcpy(col, hb + o_col, (size_t)count * 4);
  std::memcpy(dir, hb + o_dir, (size_t)count * 4);
  std::memcpy(val, hb + o_val, (size_t)count * 8);
  return 0;
}

// ------------------------------------------------------------------ objective replacement (k_objrow)
// The whole objective of `count` handles replaced (mvx_set_obj_many): handle t takes c[t*(n+1) .. ], and where it has a valid
// tableau its row 0 is rebuilt -- the weights and the base of engine_recompute_cost_row for every handle staged in the one
// pinned block of the call, one upload, one k_objrow launch for all of them.  Each handle is left as n + 1 mvx_set_obj_coef
// calls leave it; pending bound edits stay pending, as they do there.  Return codes: 0; -1 bad arguments (a null, count < 0,
// another column count, a handle listed twice); -2 device out of memory, nothing changed.
int engine_set_obj_many(mvx_prob *const *Ps, int count, const double *c) {
  if (count < 0 || (count > 0 && (!Ps || !c))) return -1;
  if (count == 0) return 0;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || Ps[t]->n != Ps[0]->n) return -1;
  {
    std::vector<const mvx_prob *> seen(Ps, Ps + count);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return -1;
  }
  const int n = Ps[0]->n;
  const size_t row = (size_t)n + 1;
  auto take = [&](int t) {
    mvx_prob *P = Ps[t];
    P->c.assign(c + (size_t)t * row, c + (size_t)(t + 1) * row);
    P->status = MVX_UNDEF;
  };
  std::vector<int> live;
  for (int t = 0; t < count; t++)
    if (Ps[t]->valid) live.push_back(t);
  if (live.empty()) {
    for (int t = 0; t < count; t++) take(t);
    return 0;
  }
  NodeCall f(NodeFlush::AtEntry, NodeResults::None);
  // up: [descriptors][w, base of each handle with a tableau]
  const size_t o_nodes = f.up(live.size() * sizeof(ObjNode));
  std::vector<size_t> o_w(live.size()), o_base(live.size());
  for (size_t k = 0; k < live.size(); k++) {
    o_w[k] = f.up((size_t)(Ps[live[k]]->m + 1) * 8);
    o_base[k] = f.up(row * 8);
  }
  if (!f.reserve()) return -2;
  for (int t = 0; t < count; t++) take(t);
  unsigned char *hb = f.hb, *db = f.db;
  ObjNode *h_nodes = (ObjNode *)(hb + o_nodes);
  for (size_t k = 0; k < live.size(); k++) {
    mvx_prob *P = Ps[live[k]];
    const int m = P->m;
    double *w = (double *)(hb + o_w[k]), *base = (double *)(hb + o_base[k]);
    w[0] = 0.0;
    for (int i = 1; i <= m; i++) w[i] = (P->bvar[i] > m) ? P->c[P->bvar[i] - m] : 0.0;
    double z = P->c[0];
    for (int j = 1; j <= n; j++) {
      const int v = P->nvar[j];
      const double cj = (v > m) ? P->c[v - m] : 0.0;
      double lb, ub;
      var_bounds(P, v, &lb, &ub);
      const double x = nb_value(P->nflag[j], lb, ub);
      base[j] = cj;
      if (x != 0.0 && cj != 0.0) z = std::fma(cj, x, z);
    }
    base[0] = z;
    h_nodes[k] = ObjNode{P->d_T, (const double *)(db + o_w[k]), (const double *)(db + o_base[k]), m, P->ld};
    P->sol_fresh = false;
    P->fresh_rows = -1;
  }
  f.upload();
  launch_objrow((const ObjNode *)(db + o_nodes), n, (int)live.size(), f.stream());
  f.fetch(); // the pinned block is free again
  return 0;
}

// ------------------------------------------------------------------ feasibility pump: rounding and objective (k_pumpobj)
// The rounding and the distance objective of `count` solved handles against root's model (mvx_pump_obj_many): one upload of
// the descriptors, the last roundings and the table of square roots, one k_pumpobj launch, one copy back.  ab[t] = (a, q):
// c_j = a * (-sg * d_j) + (q * sqrt(nnz(d))) * c0_j.  Return codes: 0; -1 bad arguments; -2 device out of memory; -3 a handle
// whose status is not MVX_OPT; -5 n > RND_NMAX, as for engine_round_many, whose model it shares.
int engine_pump_obj_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, const double *xprev, const int *has_prev,
                         const double *ab, int *info, double *xt, double *c) {
  if (!root || count < 1 || !Ps || !has_prev || !ab || !info || !xt || !c) return -1;
  const int n = root->n;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || Ps[t]->n != n || (has_prev[t] && !xprev)) return -1;
  if (n > RND_NMAX) return -5;
  for (int t = 0; t < count; t++)
    if (!Ps[t]->valid || Ps[t]->status != MVX_OPT) return -3;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  const RoundModel *M = round_model(*f.c, root);
  if (!M) return -2;
  // up: [descriptors][sqrt table][xprev]; back: [info][xt][c]; device only: [v][lo][hi]
  const size_t row = (size_t)n + 1, all = (size_t)count * row * 8;
  const size_t o_nodes = f.up((size_t)count * sizeof(PumpNode)), o_sq = f.up(row * 8), o_xp = f.up(all);
  const size_t o_info = f.out((size_t)count * 4 * 4), o_xt = f.out(all), o_c = f.out(all);
  const size_t o_v = f.dev(all), o_lo = f.dev(all), o_hi = f.dev(all);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  PumpNode *h_nodes = (PumpNode *)(hb + o_nodes);
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    PumpNode nd;
    static_cast<NodeRef &>(nd) = node_ref(P);
    nd.blb = P->d_blb; nd.bub = P->d_bub;
    nd.sg = P->dir == MVX_MIN ? -1.0 : 1.0;
    nd.a = ab[2 * (size_t)t]; nd.q = ab[2 * (size_t)t + 1];
    nd.has_prev = has_prev[t] ? 1 : 0; nd.pad = 0;
    h_nodes[t] = nd;
    double *xp = (double *)(hb + o_xp) + (size_t)t * row;
    if (has_prev[t]) std::memcpy(xp, xprev + (size_t)t * row, row * 8);
    else std::memset(xp, 0, row * 8);
  }
  double *sq = (double *)(hb + o_sq);
  for (int k = 0; k <= n; k++) sq[k] = std::sqrt((double)k);
  f.upload();
  const unsigned char *mb = (const unsigned char *)M->dev;
  PumpArgs a;
  a.nodes = (const PumpNode *)(db + o_nodes);
  a.c0 = (const double *)(mb + M->o_c);
  a.flags = (const int *)(mb + M->o_flags);
  a.xprev = (const double *)(db + o_xp);
  a.sq = (const double *)(db + o_sq);
  a.v = (double *)(db + o_v); a.lo = (double *)(db + o_lo); a.hi = (double *)(db + o_hi);
  a.info = (int *)(db + o_info); a.xt = (double *)(db + o_xt); a.c = (double *)(db + o_c);
  a.n = n; a.count = count;
  launch_pumpobj(a, f.stream());
  f.fetch();
  std::memcpy(info, hb + o_info, (size_t)count * 4 * 4);
  std::memcpy(xt, hb + o_xt, all);
  std::memcpy(c, hb + o_c, all);
  return 0;
}

// ------------------------------------------------------------------ node bound propagation (k_prop, k_setbnds)
// The second orientation of root's rounding model, rows 1..m0 by row (Ar[i][j]), next to the first: k_prop's column phase
// reads a row of consecutive columns at a time.  Built on the first propagation over this model.
static bool round_model_rows(Context &c, const mvx_prob *R, RoundModel *M) {
  if (M->dev_rows) return true;
  const int m0 = M->m0, n = M->n;
  const size_t ldn = align_up((size_t)n + 1, 64);
  std::vector<double> h((size_t)std::max(1, m0) * ldn, 0.0);
  for (int i = 1; i <= m0; i++) std::memcpy(h.data() + (size_t)(i - 1) * ldn, R->A[(size_t)i]->data(), (size_t)(n + 1) * 8);
  if (hipMalloc(&M->dev_rows, h.size() * 8) != hipSuccess) {
    (void)hipGetLastError();
    M->dev_rows = nullptr;
    g_last_error.store(MVX_ENOMEM);
    return false;
  }
  HIPCHECK(hipMemcpyAsync(M->dev_rows, h.data(), h.size() * 8, hipMemcpyHostToDevice, c.main.stream));
  HIPCHECK(hipStreamSynchronize(c.main.stream)); // the pageable source goes out of scope
  M->ldn = (int)ldn;
  return true;
}

// Node bound propagation of `count` handles over root's rows (mvx_propagate_many): the handles' bounds go up with the call
// through the node-entry arena, one k_prop launch runs every round of every handle, the final bounds come back and are
// compared with what went up.  Return codes: 0; -1 bad arguments; -2 device out of memory; -5 n > RND_NMAX.
int engine_propagate_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int max_rounds, int *infeasible, int *rounds, int *cnt,
                          int *cols, double *lb, double *ub) {
  if (!root || count < 1 || !Ps || max_rounds < 1 || !infeasible || !rounds || !cnt || !cols || !lb || !ub) return -1;
  const int n = root->n, m0 = root->m;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || Ps[t]->n != n) return -1;
  if (n > RND_NMAX) return -5;
  NodeCall f(NodeFlush::Never, NodeResults::Device);
  const RoundModel *M = round_model(*f.c, root);
  if (!M || !round_model_rows(*f.c, root, root->rmod.get())) return -2;
  // up: [lb0][ub0]; back: [lb][ub][info]; device only: the row activities when they do not fit in LDS
  const size_t nb = (size_t)count * (size_t)(n + 1) * 8;
  const size_t o_lb0 = f.up(nb), o_ub0 = f.up(nb);
  const size_t o_lb = f.out(nb), o_ub = f.out(nb), o_info = f.out((size_t)count * 8);
  const bool spill = m0 > RND_NMAX;
  const size_t o_act = f.dev(spill ? (size_t)count * 2 * (size_t)m0 * 8 : 0), o_actk = f.dev(spill ? (size_t)count * (size_t)m0 * 4 : 0);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  for (int t = 0; t < count; t++) {
    std::memcpy(hb + o_lb0 + (size_t)t * (size_t)(n + 1) * 8, Ps[t]->clb.data(), (size_t)(n + 1) * 8);
    std::memcpy(hb + o_ub0 + (size_t)t * (size_t)(n + 1) * 8, Ps[t]->cub.data(), (size_t)(n + 1) * 8);
  }
  f.upload();
  const unsigned char *mb = (const unsigned char *)M->dev;
  PropArgs a;
  a.At = (const double *)mb;
  a.Ar = (const double *)M->dev_rows;
  a.rlo = (const double *)(mb + M->o_rlo); a.rhi = (const double *)(mb + M->o_rhi);
  a.flags = (const int *)(mb + M->o_flags);
  a.lb0 = (const double *)(db + o_lb0); a.ub0 = (const double *)(db + o_ub0);
  a.lb = (double *)(db + o_lb); a.ub = (double *)(db + o_ub); a.info = (int *)(db + o_info);
  a.act = spill ? (double *)(db + o_act) : nullptr;
  a.actk = spill ? (int *)(db + o_actk) : nullptr;
  a.n = n; a.m0 = m0; a.ldm = M->ldm; a.ldn = M->ldn; a.max_rounds = max_rounds; a.count = count;
  launch_prop(a, f.stream());
  f.fetch();
  const int *h_info = (const int *)(hb + o_info);
  for (int t = 0; t < count; t++) {
    const double *l0 = Ps[t]->clb.data(), *u0 = Ps[t]->cub.data();
    const double *l1 = (const double *)(hb + o_lb) + (size_t)t * (size_t)(n + 1), *u1 = (const double *)(hb + o_ub) + (size_t)t * (size_t)(n + 1);
    infeasible[t] = h_info[2 * t];
    rounds[t] = h_info[2 * t + 1];
    int k = 0;
    if (!infeasible[t])
      for (int j = 1; j <= n; j++)
        if (l1[j] != l0[j] || u1[j] != u0[j]) {
          const size_t o = (size_t)t * (size_t)n + (size_t)k++;
          cols[o] = j;
          lb[o] = l1[j];
          ub[o] = u1[j];
        }
    cnt[t] = k;
  }
  return 0;
}

// ------------------------------------------------------------------ conflict graph (k_conflict_rows, k_conflict)
// The conflict graph of the binary columns of `R` (mvx_conflict_graph): the model is the one k_prop reads (both orientations,
// uploaded on first use and kept with the handle), nothing goes up with the call, two launches, the words come back and the
// edges are counted here.  Return codes: 0; -1 bad arguments; -2 device out of memory.
int engine_conflict_graph(const mvx_prob *R, unsigned long long *adj, long long *edges) {
  if (!R || !adj || !edges) return -1;
  const int n = R->n, m0 = R->m;
  NodeCall f(NodeFlush::Never, NodeResults::Device);
  const RoundModel *M = round_model(*f.c, R);
  if (!M || !round_model_rows(*f.c, R, R->rmod.get())) return -2;
  const size_t W = ((size_t)n + 1 + 63) / 64, words = ((size_t)n + 1) * W;
  // back: [adj]; device only: [rowinfo]
  const size_t o_adj = f.out(words * 8);
  const size_t o_info = f.dev((size_t)std::max(1, m0) * 4 * 8);
  if (!f.reserve()) return -2;
  const unsigned char *mb = (const unsigned char *)M->dev;
  ConflictArgs a;
  a.At = (const double *)mb;
  a.Ar = (const double *)M->dev_rows;
  a.rlo = (const double *)(mb + M->o_rlo); a.rhi = (const double *)(mb + M->o_rhi);
  a.clo = (const double *)(mb + M->o_clo); a.chi = (const double *)(mb + M->o_chi);
  a.flags = (const int *)(mb + M->o_flags);
  a.rowinfo = (double *)(f.db + o_info);
  a.adj = (unsigned long long *)(f.db + o_adj);
  a.n = n; a.m0 = m0; a.ldm = M->ldm; a.ldn = M->ldn; a.W = (int)W; a.pad = 0;
  launch_conflict(a, f.stream());
  f.fetch();
  std::memcpy(adj, f.hb + o_adj, words * 8);
  long long bits = 0;
  for (size_t w = 0; w < words; w++) bits += __builtin_popcountll(adj[w]);
  *edges = bits / 2;
  return 0;
}

// ------------------------------------------------------------------ clique cuts in the tree (k_cliquemembers, k_cliquesep)
// The conflict graph of root's rounding model on the device, next to the model and gone with it (round_model_current): computed
// by k_conflict_rows / k_conflict on the first separation over this model, with the columns that have a neighbour.  The row
// numbers k_conflict_rows leaves for k_conflict live behind the graph in the same allocation.
static bool round_model_graph(Context &c, RoundModel *M) {
  if (M->dev_graph) return true;
  const int n = M->n, m0 = M->m0;
  const size_t W = ((size_t)n + 1 + 63) / 64;
  Carver carve;
  carve(((size_t)n + 1) * W * 8);
  M->o_member = carve(((size_t)n + 1) * 4);
  const size_t o_info = carve((size_t)std::max(1, m0) * 4 * 8);
  if (hipMalloc(&M->dev_graph, carve.off) != hipSuccess) {
    (void)hipGetLastError();
    M->dev_graph = nullptr;
    g_last_error.store(MVX_ENOMEM);
    return false;
  }
  const unsigned char *mb = (const unsigned char *)M->dev;
  unsigned char *gb = (unsigned char *)M->dev_graph;
  ConflictArgs a;
  a.At = (const double *)mb;
  a.Ar = (const double *)M->dev_rows;
  a.rlo = (const double *)(mb + M->o_rlo); a.rhi = (const double *)(mb + M->o_rhi);
  a.clo = (const double *)(mb + M->o_clo); a.chi = (const double *)(mb + M->o_chi);
  a.flags = (const int *)(mb + M->o_flags);
  a.rowinfo = (double *)(gb + o_info);
  a.adj = (unsigned long long *)gb;
  a.n = n; a.m0 = m0; a.ldm = M->ldm; a.ldn = M->ldn; a.W = (int)W; a.pad = 0;
  launch_conflict(a, c.main.stream);
  launch_clique_members(a.adj, (int *)(gb + M->o_member), n, (int)W, c.main.stream);
  return true;
}

// The clique separation of `count` solved handles against root's conflict graph (mvx_clique_cuts_many): the descriptors go up,
// one k_cliquesep launch, the counts, sets and sums come back once.  No handle is changed.  Return codes: 0; -1 bad arguments;
// -2 device out of memory, nothing written; -3 a handle whose status is not MVX_OPT; -5 n > RND_NMAX.
int engine_clique_cuts_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int max_cuts, int *cnt, unsigned long long *q,
                            double *sum) {
  if (!root || count < 0 || max_cuts < 1 || max_cuts > CLQ_KMAX) return -1;
  if (count == 0) return 0;
  if (!Ps || !cnt || !q || !sum) return -1;
  const int n = root->n;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || Ps[t]->n != n) return -1;
  if (n > RND_NMAX) return -5;
  for (int t = 0; t < count; t++)
    if (!Ps[t]->valid || Ps[t]->status != MVX_OPT) return -3;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  const RoundModel *M = round_model(*f.c, root);
  if (!M || !round_model_rows(*f.c, root, root->rmod.get()) || !round_model_graph(*f.c, root->rmod.get())) return -2;
  const size_t W = ((size_t)n + 1 + 63) / 64, slots = (size_t)count * (size_t)max_cuts;
  // up: [descriptors]; back: [cnt][sum][q]
  const size_t o_nodes = f.up((size_t)count * sizeof(NodeRef));
  const size_t o_cnt = f.out((size_t)count * 4), o_sum = f.out(slots * 8), o_q = f.out(slots * W * 8);
  if (!f.reserve()) return -2;
  NodeRef *h_nodes = (NodeRef *)(f.hb + o_nodes);
  for (int t = 0; t < count; t++) h_nodes[t] = node_ref(Ps[t]);
  f.upload();
  const unsigned char *gb = (const unsigned char *)M->dev_graph;
  CliqueArgs a;
  a.nodes = (const NodeRef *)(f.db + o_nodes);
  a.adj = (const unsigned long long *)gb;
  a.member = (const int *)(gb + M->o_member);
  a.cnt = (int *)(f.db + o_cnt);
  a.sum = (double *)(f.db + o_sum);
  a.q = (unsigned long long *)(f.db + o_q);
  a.n = n; a.W = (int)W; a.max_cuts = max_cuts; a.count = count;
  launch_cliquesep(a, f.stream());
  f.fetch();
  // the kernel writes the kept slots only: the others are zero here
  std::memcpy(cnt, f.hb + o_cnt, (size_t)count * 4);
  std::memset(q, 0, slots * W * 8);
  std::memset(sum, 0, slots * 8);
  for (int t = 0; t < count; t++) {
    const size_t o = (size_t)t * (size_t)max_cuts, k = (size_t)cnt[t];
    std::memcpy(q + o * W, f.hb + o_q + o * W * 8, k * W * 8);
    std::memcpy(sum + o, f.hb + o_sum + o * 8, k * 8);
  }
  return 0;
}

// ------------------------------------------------------------------ KKT check (k_kkt_vals, k_kkt_rows, k_kkt_cols, k_kkt_fin)
// The KKT conditions of `count` solved handles against their own models (mvx_kkt_many, DESIGN.md "KKT check (kkt)"): rows 1..m0
// are read from root's rounding model in both orientations (uploaded on first use, checked on every call), each handle's cut
// rows m0+1..m and, where it differs from root's, its objective go up with the descriptors in the call's one upload, and the
// values, duals, statuses and bounds are read where they lie in each handle's slab.  One flush of the recorded clones, one
// upload, one launch sequence, one copy back; no handle is changed.  r_pe / r_de (nullable): the residual vectors of handle 0,
// which the single-handle entry asks for.  Return codes: 0; -1 bad arguments; -2 device out of memory, nothing written; -3 a
// handle that is MVX_UNDEF or has no tableau (or bound edits still pending), or one whose first m0 rows are not root's.
int engine_kkt_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, double *val, int *ind, double *r_pe, double *r_de) {
  if (!root || count < 0) return -1;
  if (count == 0) return 0;
  if (!Ps || !val || !ind) return -1;
  const int n = root->n, m0 = root->m;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || Ps[t]->n != n) return -1;
  if (n < 1 || m0 < 1) return -3;
  size_t vars = 0, cut_rows = 0, own_obj = 0;
  int mmax = 0;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    if (!P->valid || P->status == MVX_UNDEF || !P->pending.empty() || P->m < m0) return -3;
    if (P != root)
      for (int i = 1; i <= m0; i++)
        if (P->A[(size_t)i].get() != root->A[(size_t)i].get()) return -3;
    vars += (size_t)P->m + (size_t)n + 1;
    cut_rows += (size_t)(P->m - m0);
    own_obj += P != root && P->c != root->c;
    mmax = std::max(mmax, P->m);
  }
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  const RoundModel *M = round_model(*f.c, root);
  if (!M || !round_model_rows(*f.c, root, root->rmod.get())) return -2;
  const size_t row = (size_t)n + 1;
  const bool want_r = r_pe || r_de;
  // up: [descriptors][cut rows][own objectives]; back: [val][ind] (and the residuals when they are wanted); device only: the
  // by-variable arrays
  const size_t o_nodes = f.up((size_t)count * sizeof(KktNode)), o_cuts = f.up(cut_rows * row * 8), o_obj = f.up(own_obj * row * 8);
  const size_t o_val = f.out((size_t)count * 8 * 8), o_ind = f.out((size_t)count * 8 * 4);
  const size_t o_res = want_r ? f.out(vars * 8) : f.dev(vars * 8);
  const size_t o_x = f.dev(vars * 8), o_du = f.dev(vars * 8), o_lo = f.dev(vars * 8), o_up = f.dev(vars * 8), o_st = f.dev(vars * 4);
  size_t o_term[8];
  for (int k = 0; k < 8; k++) o_term[k] = f.dev(vars * 8);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  KktNode *h_nodes = (KktNode *)(hb + o_nodes);
  size_t voff = 0, cut_at = 0, obj_at = 0;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    KktNode &nd = h_nodes[t];
    static_cast<NodeRef &>(nd) = node_ref(P);
    nd.blb = P->d_blb;
    nd.bub = P->d_bub;
    nd.cuts = nullptr;
    nd.c = nullptr;
    if (P->m > m0) {
      nd.cuts = (const double *)(db + o_cuts) + cut_at * row;
      for (int i = m0 + 1; i <= P->m; i++, cut_at++) {
        if (P->A[(size_t)i]) std::memcpy(hb + o_cuts + cut_at * row * 8, P->A[(size_t)i]->data(), row * 8);
        else std::memset(hb + o_cuts + cut_at * row * 8, 0, row * 8); // a row that was never filled is empty
      }
    }
    if (P != root && P->c != root->c) {
      nd.c = (const double *)(db + o_obj) + obj_at * row;
      std::memcpy(hb + o_obj + (obj_at++) * row * 8, P->c.data(), row * 8);
    }
    nd.voff = voff;
    nd.sg = P->dir == MVX_MIN ? 1.0 : -1.0;
    voff += (size_t)P->m + row;
  }
  f.upload();
  const unsigned char *mb = (const unsigned char *)M->dev;
  KktArgs a;
  a.nodes = (const KktNode *)(db + o_nodes);
  a.At = (const double *)mb;
  a.Ar = (const double *)M->dev_rows;
  a.c0 = (const double *)(mb + M->o_c);
  a.x = (double *)(db + o_x); a.du = (double *)(db + o_du); a.lo = (double *)(db + o_lo); a.up = (double *)(db + o_up);
  a.res = (double *)(db + o_res);
  a.st = (int *)(db + o_st);
  for (int k = 0; k < 8; k++) a.term[k] = (double *)(db + o_term[k]);
  a.val = (double *)(db + o_val); a.ind = (int *)(db + o_ind);
  a.n = n; a.m0 = m0; a.ldm = M->ldm; a.ldn = M->ldn; a.count = count; a.mmax = mmax;
  launch_kkt(a, f.stream());
  f.copy_back(want_r ? o_res + ((size_t)Ps[0]->m + row) * 8 : 0); // of the residuals, handle 0's slice only
  f.sync();
  std::memcpy(val, hb + o_val, (size_t)count * 8 * 8);
  std::memcpy(ind, hb + o_ind, (size_t)count * 8 * 4);
  const double *h_res = (const double *)(hb + o_res);
  if (r_pe) {
    r_pe[0] = 0.0;
    std::memcpy(r_pe + 1, h_res + 1, (size_t)Ps[0]->m * 8);
  }
  if (r_de) {
    r_de[0] = 0.0;
    std::memcpy(r_de + 1, h_res + (size_t)Ps[0]->m + 1, (size_t)n * 8);
  }
  return 0;
}

// ------------------------------------------------- Farkas proof (k_farkas_rows, k_farkas_pick, k_farkas_vars, k_farkas_cols, k_farkas_fin)
// A proof of infeasibility for `count` handles against their own models (mvx_farkas_many, DESIGN.md "Infeasibility and unboundedness
// proofs (farkas)"): one pass over each handle's tableau slab finds the row that proves, its weights are evaluated on the columns
// of root's rounding model (uploaded on first use, checked on every call) and on the handle's cut rows m0+1..m, which go up with
// the descriptors in the call's one upload.  One flush of the recorded clones, one upload, one launch sequence, one copy back; no
// handle is changed.  y (nullable): the row weights of handle 0, which the single-handle entry asks for.  Return codes: 0; -1 bad
// arguments; -2 device out of memory, nothing written; -3 a handle that is MVX_UNDEF or has no tableau (or bound edits still
// pending), or one whose first m0 rows are not root's.
int engine_farkas_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, double *val, int *ind, double *y) {
  if (!root || count < 0) return -1;
  if (count == 0) return 0;
  if (!Ps || !val || !ind) return -1;
  const int n = root->n, m0 = root->m;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || Ps[t]->n != n) return -1;
  if (n < 1 || m0 < 1) return -3;
  size_t vars = 0, cut_rows = 0, rows = 0;
  int mmax = 0;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    if (!P->valid || P->status == MVX_UNDEF || !P->pending.empty() || P->m < m0) return -3;
    if (P != root)
      for (int i = 1; i <= m0; i++)
        if (P->A[(size_t)i].get() != root->A[(size_t)i].get()) return -3;
    vars += (size_t)P->m + (size_t)n + 1;
    rows += (size_t)P->m;
    cut_rows += (size_t)(P->m - m0);
    mmax = std::max(mmax, P->m);
  }
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  const RoundModel *M = round_model(*f.c, root);
  if (!M) return -2;
  const size_t row = (size_t)n + 1;
  // up: [descriptors][cut rows]; back: [val][ind] (and the form by variable when y is wanted); device only: the row records, the
  // picks and the other by-variable arrays
  const size_t o_nodes = f.up((size_t)count * sizeof(FkNode)), o_cuts = f.up(cut_rows * row * 8);
  const size_t o_val = f.out((size_t)count * 4 * 8), o_ind = f.out((size_t)count * 4 * 4);
  const size_t o_f = y ? f.out(vars * 8) : f.dev(vars * 8);
  const size_t o_g = f.dev(vars * 8), o_lo = f.dev(vars * 8), o_up = f.dev(vars * 8), o_dt = f.dev(vars * 8);
  const size_t o_rrel = f.dev(rows * 2 * 8), o_pick = f.dev((size_t)count * 4);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  FkNode *h_nodes = (FkNode *)(hb + o_nodes);
  size_t voff = 0, roff = 0, cut_at = 0;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    FkNode &nd = h_nodes[t];
    static_cast<NodeRef &>(nd) = node_ref(P);
    nd.blb = P->d_blb;
    nd.bub = P->d_bub;
    nd.cuts = nullptr;
    if (P->m > m0) {
      nd.cuts = (const double *)(db + o_cuts) + cut_at * row;
      for (int i = m0 + 1; i <= P->m; i++, cut_at++) {
        if (P->A[(size_t)i]) std::memcpy(hb + o_cuts + cut_at * row * 8, P->A[(size_t)i]->data(), row * 8);
        else std::memset(hb + o_cuts + cut_at * row * 8, 0, row * 8); // a row that was never filled is empty
      }
    }
    nd.voff = voff;
    nd.roff = roff;
    voff += (size_t)P->m + row;
    roff += 2 * (size_t)P->m;
  }
  f.upload();
  FkArgs a;
  a.nodes = (const FkNode *)(db + o_nodes);
  a.At = (const double *)M->dev;
  a.rrel = (double *)(db + o_rrel);
  a.f = (double *)(db + o_f); a.g = (double *)(db + o_g); a.lo = (double *)(db + o_lo); a.up = (double *)(db + o_up);
  a.dterm = (double *)(db + o_dt);
  a.pick = (int *)(db + o_pick);
  a.val = (double *)(db + o_val); a.ind = (int *)(db + o_ind);
  a.n = n; a.m0 = m0; a.ldm = M->ldm; a.count = count; a.mmax = mmax;
  launch_farkas(a, f.stream());
  f.copy_back(y ? o_f + ((size_t)Ps[0]->m + 1) * 8 : 0); // of the form, handle 0's row weights only
  f.sync();
  std::memcpy(val, hb + o_val, (size_t)count * 4 * 8);
  std::memcpy(ind, hb + o_ind, (size_t)count * 4 * 4);
  if (y) {
    y[0] = 0.0;
    std::memcpy(y + 1, hb + o_f + 8, (size_t)Ps[0]->m * 8);
  }
  return 0;
}

// ------------------------------------------------------- the unbounded ray (k_ray_cols, k_ray_pick, k_ray_vars, k_ray_rows, k_ray_fin)
// The ray that proves a handle unbounded (mvx_ray, same section of DESIGN.md): one pass down the columns of the slab finds the
// position, the ray is checked against the handle's own rows by row (the second orientation of its rounding model) and its
// objective, which goes up with the call.  No handle is changed.  d (nullable): the ray by variable.  Return codes: 0; -1 bad
// arguments; -2 device out of memory, nothing written; -3 a handle that is MVX_UNDEF or has no tableau (or bound edits pending).
int engine_ray(const mvx_prob *P, double *val, int *ind, double *d) {
  if (!P || !val || !ind) return -1;
  const int n = P->n, m = P->m;
  if (n < 1 || m < 1 || !P->valid || P->status == MVX_UNDEF || !P->pending.empty()) return -3;
  NodeCall f(NodeFlush::AtEntry, NodeResults::Device);
  const RoundModel *M = round_model(*f.c, P);
  if (!M || !round_model_rows(*f.c, P, P->rmod.get())) return -2;
  const size_t vars = (size_t)m + (size_t)n + 1;
  const size_t o_c = f.up(((size_t)n + 1) * 8);
  const size_t o_val = f.out(4 * 8), o_ind = f.out(6 * 4);
  const size_t o_d = d ? f.out(vars * 8) : f.dev(vars * 8);
  const size_t o_lo = f.dev(vars * 8), o_up = f.dev(vars * 8), o_rae = f.dev(((size_t)m + 1) * 8), o_rre = f.dev(((size_t)m + 1) * 8);
  const size_t o_open = f.dev(((size_t)n + 1) * 4), o_pick = f.dev(4);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  std::memcpy(hb + o_c, P->c.data(), ((size_t)n + 1) * 8);
  f.upload();
  RayArgs a;
  a.nd = node_ref(P);
  a.blb = P->d_blb;
  a.bub = P->d_bub;
  a.Ar = (const double *)M->dev_rows;
  a.c = (const double *)(db + o_c);
  a.open = (int *)(db + o_open);
  a.pick = (int *)(db + o_pick);
  a.d = (double *)(db + o_d); a.lo = (double *)(db + o_lo); a.up = (double *)(db + o_up);
  a.rae = (double *)(db + o_rae); a.rre = (double *)(db + o_rre);
  a.val = (double *)(db + o_val); a.ind = (int *)(db + o_ind);
  a.sg = P->dir == MVX_MIN ? 1.0 : -1.0;
  a.n = n; a.ldn = M->ldn;
  launch_ray(a, f.stream());
  f.fetch();
  std::memcpy(val, hb + o_val, 4 * 8);
  std::memcpy(ind, hb + o_ind, 6 * 4);
  if (d) {
    d[0] = 0.0;
    std::memcpy(d + 1, hb + o_d + 8, (vars - 1) * 8);
  }
  return 0;
}

// ------------------------------------------------------------------ incumbent polishing (k_lsact, k_lsmove, k_lsapply)
// The exchange search of mvx_polish_many on `count` points against root's model (both orientations, as the conflict graph
// reads it): the points go up, k_lsact takes the entry, then iterations (k_lsmove + k_lsapply) are enqueued LS_GROUP at a time
// with one look at the done flags per group, never more than max_moves in all, k_lsact again for the end, and the results come
// back.  No handle is read or changed.  The points go through in chunks that keep the records (2n per point) within 256 MiB
// and the grid's second dimension within its limit; the arena is reserved once for all of them, so -2 leaves nothing written.
// Return codes: 0; -1 bad arguments; -2 device out of memory.  The kernels have no size limit.
int engine_polish_many(const mvx_prob *root, int count, double *x, int max_moves, double *obj, int *moves, int *ok) {
  if (!root || count < 0 || max_moves < 1 || max_moves > 100000 || (count > 0 && (!x || !obj || !moves || !ok))) return -1;
  if (count == 0) return 0;
  const int n = root->n, m0 = root->m;
  NodeCall f(NodeFlush::Never, NodeResults::Device);
  const RoundModel *M = round_model(*f.c, root);
  if (!M || !round_model_rows(*f.c, root, root->rmod.get())) return -2;
  const size_t row = (size_t)n + 1, recs = (size_t)std::max(1, 2 * n) * sizeof(LsRec);
  const int chunk = (int)std::min<size_t>((size_t)count, std::max<size_t>(1, std::min<size_t>(4096, ((size_t)256 << 20) / recs)));
  // up: [xin]; back: [x][obj][moves][ok][done]; device only: [r][obj0][records]
  const size_t o_xin = f.up((size_t)chunk * row * 8);
  const size_t o_x = f.out((size_t)chunk * row * 8), o_obj = f.out((size_t)chunk * 8), o_moves = f.out((size_t)chunk * 4);
  const size_t o_ok = f.out((size_t)chunk * 4), o_done = f.out((size_t)chunk * 4);
  const size_t o_r = f.dev((size_t)chunk * (size_t)M->ldm * 8), o_obj0 = f.dev((size_t)chunk * 8), o_rec = f.dev((size_t)chunk * recs);
  if (!f.reserve()) return -2;
  unsigned char *hb = f.hb, *db = f.db;
  const unsigned char *mb = (const unsigned char *)M->dev;
  LsArgs a;
  a.At = (const double *)mb;
  a.Ar = (const double *)M->dev_rows;
  a.rlo = (const double *)(mb + M->o_rlo); a.rhi = (const double *)(mb + M->o_rhi);
  a.clo = (const double *)(mb + M->o_clo); a.chi = (const double *)(mb + M->o_chi); a.c = (const double *)(mb + M->o_c);
  a.flags = (const int *)(mb + M->o_flags);
  a.xin = (const double *)(db + o_xin); a.x = (double *)(db + o_x); a.r = (double *)(db + o_r);
  a.obj = (double *)(db + o_obj); a.obj0 = (double *)(db + o_obj0);
  a.moves = (int *)(db + o_moves); a.ok = (int *)(db + o_ok); a.done = (int *)(db + o_done);
  a.rec = (LsRec *)(db + o_rec);
  a.sg = root->dir == MVX_MIN ? -1.0 : 1.0;
  a.n = n; a.m0 = m0; a.ldm = M->ldm; a.ldn = M->ldn; a.pad = 0;
  for (int t0 = 0; t0 < count; t0 += chunk) {
    const int k = std::min(chunk, count - t0);
    a.count = k;
    std::memcpy(hb + o_xin, x + (size_t)t0 * row, (size_t)k * row * 8);
    f.upload();
    launch_lsact(a, 0, f.stream());
    const int *h_done = (const int *)(hb + o_done);
    for (int queued = 0; queued < max_moves;) {
      const int g = std::min(LS_GROUP, max_moves - queued);
      for (int q = 0; q < g; q++) launch_lsiter(a, f.stream());
      queued += g;
      HIPCHECK(hipMemcpyAsync(hb + o_done, db + o_done, (size_t)k * 4, hipMemcpyDeviceToHost, f.stream()));
      f.sync();
      bool all = true;
      for (int t = 0; t < k; t++) all = all && h_done[t] != 0;
      if (all) break;
    }
    launch_lsact(a, 1, f.stream());
    f.fetch();
    const double *h_x = (const double *)(hb + o_x), *h_obj = (const double *)(hb + o_obj);
    const int *h_moves = (const int *)(hb + o_moves), *h_ok = (const int *)(hb + o_ok);
    for (int t = 0; t < k; t++) {
      const size_t g = (size_t)(t0 + t);
      ok[g] = h_ok[t];
      obj[g] = h_ok[t] ? h_obj[t] : 0.0;
      moves[g] = h_ok[t] ? h_moves[t] : 0;
      if (h_ok[t]) std::memcpy(x + g * row + 1, h_x + (size_t)t * row + 1, (size_t)n * 8); // a refused point stays untouched
    }
  }
  return 0;
}

// ------------------------------------------------------------------ bound lists (k_setbnds)
// What the two bound-list entries check alike, before anything is edited: 1 go on, 0 nothing to do, -1 a bad list.  `general`
// (mvx_set_col_bnds_many): infinite bounds are allowed, a handle listed twice is not; else (mvx_tighten_cols_many) the
// reverse.
static int check_bound_lists(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub, bool general) {
  if (count < 0 || (count > 0 && (!Ps || !off))) return -1;
  if (count == 0) return 0;
  if (off[0] < 0) return -1;
  std::unordered_set<const mvx_prob *> seen;
  for (int t = 0; t < count; t++)
    if (!Ps[t] || off[t + 1] < off[t] || (general && !seen.insert(Ps[t]).second)) return -1;
  if (off[count] == off[0]) return 0;
  if (!cols || !lb || !ub) return -1;
  const double inf = std::numeric_limits<double>::infinity();
  for (int t = 0; t < count; t++) {
    int prev = 0;
    for (int k = off[t]; k < off[t + 1]; k++) {
      const int j = cols[k];
      const bool ok = general ? lb[k] <= ub[k] && lb[k] != inf && ub[k] != -inf : std::isfinite(lb[k]) && std::isfinite(ub[k]) && lb[k] <= ub[k];
      if (j < 1 || j > Ps[t]->n || j <= prev || !ok) return -1;
      prev = j;
    }
  }
  return 1;
}

// Checked bound lists of many handles with one launch.  Each entry does on the host what mvx_set_col_bnds + engine_apply_bounds
// do, in list order -- the model, the nflag mirror, the pending edits of basic rows (merged by row; flushed when the ninth
// arrives), hint_dual, status -- and what they would have launched is collected: bound writes (one per row or position and
// handle: the last one the ordered launches would have made) and shifts of column 0, which leave as one k_setbnds launch.
static int apply_bound_lists(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub) {
  std::vector<SetbHandle> hs;
  std::vector<SetbEntry> es;
  std::vector<SetbShift> ss;
  bool device = false; // a handle without a tableau is a model edit only, as in mvx_set_col_bnds: no engine call
  for (int t = 0; t < count; t++) device = device || (Ps[t]->valid && off[t + 1] > off[t]);
  NodeCall f(NodeFlush::BeforeUpload, NodeResults::None, device);
  // laid out for the most the lists can ask for, so that out of memory is known before anything is edited
  const size_t total = (size_t)(off[count] - off[0]);
  const size_t o_hs = f.up((size_t)count * sizeof(SetbHandle)), o_es = f.up((total + (size_t)count * MAX_EDITS) * sizeof(SetbEntry)),
               o_ss = f.up(total * sizeof(SetbShift));
  if (device && !f.reserve()) return -2;
  for (int t = 0; t < count; t++) {
    mvx_prob *P = Ps[t];
    if (off[t + 1] == off[t]) continue;
    SetbHandle h{P->d_T, P->d_blb, P->d_bub, P->d_nlb, P->d_nub, P->d_nflag, P->ld, P->m, (int)es.size(), 0, (int)ss.size(), 0};
    // A row can be sent twice by one list: a pending edit of column j's row goes out with the first eight, j's own entry
    // queues the row again and a later overflow sends it.  The per-entry path's launches are ordered, so the later bounds
    // win; the lanes of one launch are not, so each row has ONE entry per handle and a later flush overwrites it.
    std::unordered_map<int, size_t> sent; // row -> its entry in es
    for (int k = off[t]; k < off[t + 1]; k++) {
      const int j = cols[k];
      const bool has_l = std::isfinite(lb[k]), has_u = std::isfinite(ub[k]);
      const int type = has_l && has_u ? (lb[k] == ub[k] ? MVX_FX : MVX_DB) : has_l ? MVX_LO : has_u ? MVX_UP : MVX_FR;
      const double olb = P->clb[(size_t)j], oub = P->cub[(size_t)j];
      P->ctype[(size_t)j] = type;
      P->clb[(size_t)j] = lb[k];
      P->cub[(size_t)j] = ub[k];
      if (!P->valid) continue;
      const int pos = P->pos[(size_t)(P->m + j)];
      if (pos > 0) {
        bool merged = false;
        for (auto &e : P->pending)
          if (e.row == pos) {
            e.lb = lb[k];
            e.ub = ub[k];
            merged = true;
          }
        if (!merged) {
          if ((int)P->pending.size() == MAX_EDITS) {
            for (const auto &e : P->pending) {
              auto it = sent.find(e.row);
              if (it != sent.end()) {
                es[it->second].lb = e.lb;
                es[it->second].ub = e.ub;
              } else {
                sent.emplace(e.row, es.size());
                es.push_back(SetbEntry{e.lb, e.ub, e.row, -1});
              }
            }
            P->pending.clear();
          }
          P->pending.push_back({pos, lb[k], ub[k]});
        }
        P->hint_dual = true;
      } else {
        const int jj = -pos;
        const double xo = nb_value(P->nflag[(size_t)jj], olb, oub);
        const int flag = type == MVX_FR ? MVX_NF : type == MVX_LO ? MVX_NL : type == MVX_UP ? MVX_NU
                         : type == MVX_DB ? (P->nflag[(size_t)jj] == MVX_NU ? MVX_NU : MVX_NL) : MVX_NS;
        P->nflag[(size_t)jj] = flag;
        es.push_back(SetbEntry{lb[k], ub[k], jj, flag});
        const double xn = nb_value(flag, lb[k], ub[k]);
        if (xn != xo) ss.push_back(SetbShift{xn - xo, jj, 0});
      }
    }
    P->status = MVX_UNDEF;
    if (!P->valid) continue;
    P->sol_fresh = false;
    P->fresh_rows = -1;
    h.e1 = (int)es.size();
    h.s1 = (int)ss.size();
    if (h.e1 > h.e0 || h.s1 > h.s0) hs.push_back(h);
  }
  if (hs.empty()) return 0;
  std::memcpy(f.hb + o_hs, hs.data(), hs.size() * sizeof(SetbHandle));
  if (!es.empty()) std::memcpy(f.hb + o_es, es.data(), es.size() * sizeof(SetbEntry));
  if (!ss.empty()) std::memcpy(f.hb + o_ss, ss.data(), ss.size() * sizeof(SetbShift));
  f.upload(); // behind the recorded clones: a clone INTO one of these slabs must land before the edits do
  launch_setbnds((const SetbHandle *)(f.db + o_hs), (const SetbEntry *)(f.db + o_es), (const SetbShift *)(f.db + o_ss), (int)hs.size(), f.stream());
  f.fetch();
  return 0;
}

// General bound lists of many handles (mvx_set_col_bnds_many): -1 changes nothing.
int engine_set_bounds_many(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub) {
  const int rc = check_bound_lists(Ps, count, off, cols, lb, ub, true);
  return rc <= 0 ? rc : apply_bound_lists(Ps, count, off, cols, lb, ub);
}

// Bound lists that tighten columns where they rest (mvx_tighten_cols_many): finite bounds on non-basic columns whose resting
// value stays put -- -1 and -4 change nothing -- so the shared edit queues bound writes only: no pending row edits, no shifts
// of column 0, the tableau is not touched.  A handle may be listed twice (with disjoint columns).
int engine_tighten_many(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub) {
  const int rc = check_bound_lists(Ps, count, off, cols, lb, ub, false);
  if (rc <= 0) return rc;
  for (int t = 0; t < count; t++) {
    const mvx_prob *P = Ps[t];
    if (!P->valid) continue;
    for (int k = off[t]; k < off[t + 1]; k++) {
      const int j = cols[k], pos = P->pos[(size_t)(P->m + j)];
      if (pos > 0) return -4;
      const int flag = lb[k] == ub[k] ? MVX_NS : (P->nflag[(size_t)-pos] == MVX_NU ? MVX_NU : MVX_NL);
      if (nb_value(flag, lb[k], ub[k]) != nb_value(P->nflag[(size_t)-pos], P->clb[(size_t)j], P->cub[(size_t)j])) return -4;
    }
  }
  return apply_bound_lists(Ps, count, off, cols, lb, ub);
}

// ------------------------------------------------------------------ pack / unpack (migration)
// Device-side image of a handle for node migration between ranks:
//   [PackHdr][ctype,rtype,bvar,nvar,nflag i32][clb,cub,rlb,rub f64][model rows m_base+1..m, n+1 f64 each] pad 256
//   | T live rows | slab tail
// Rows 1..m_base of the model are the receiver's own (its copy of the root problem); the rows appended since
// (GMI cut rows, cut.cpp:23-43) travel densely with the image.
struct PackHdr {
  long long magic, m, n, ld, m_cap, status, it_cnt, valid, hint_dual, host_bytes, m_base, reserved;
  double last_tol[3];
  double pad_;
};
static const long long PACK_MAGIC = 0x4d56584849504cll;

static size_t pack_host_bytes(int m, int n, int m_base) {
  size_t sz = sizeof(PackHdr);
  sz += sizeof(int) * ((size_t)(n + 1) + 2 * (size_t)(m + 1) + 2 * (size_t)(n + 1));
  sz = align_up(sz, 8);
  sz += sizeof(double) * (2 * (size_t)(n + 1) + 2 * (size_t)(m + 1));
  sz += sizeof(double) * (size_t)(m - m_base) * (size_t)(n + 1);
  return align_up(sz, 256);
}

long long engine_pack_size(const mvx_prob *P, int m_base) {
  if (m_base < 0 || m_base > P->m) return -1;
  size_t sz = pack_host_bytes(P->m, P->n, m_base);
  if (P->valid) {
    SlabLayout L = slab_layout(P->m_cap, P->ld);
    sz += align_up((size_t)(P->m + 1) * P->ld * 8, 256) + (L.total - L.o_bvar);
  }
  return (long long)sz;
}

int engine_pack(const mvx_prob *P, int m_base, void *dev_buf) {
  if (m_base < 0 || m_base > P->m) return -1;
  Context &c = ctx();
  MAIN_LOCK(c);
  SolveCtx &sc = c.main;
  flush_copies(c);
  if (P->valid) flush_edits(sc, const_cast<mvx_prob *>(P)); // the image carries the device-side bounds
  const int m = P->m, n = P->n;
  const size_t hb = pack_host_bytes(m, n, m_base);
  std::vector<unsigned char> host(hb, 0);
  unsigned char *b = host.data();
  PackHdr h{};
  // a handle without a tableau has no slab: whatever geometry its fields still hold is not part of its image
  h.magic = PACK_MAGIC; h.m = m; h.n = n; h.ld = P->valid ? P->ld : 0; h.m_cap = P->valid ? P->m_cap : 0; h.status = P->status;
  h.it_cnt = P->it_cnt; h.valid = P->valid; h.hint_dual = P->hint_dual; h.host_bytes = (long long)hb; h.m_base = m_base; h.reserved = P->piv_since_check;
  std::memcpy(h.last_tol, P->last_tol, sizeof(h.last_tol));
  std::memcpy(b, &h, sizeof(h));
  b += sizeof(h);
  unsigned char *b0 = b;
  auto put = [&](const void *src, size_t bytes) {
    if (src) std::memcpy(b, src, bytes);
    b += bytes;
  };
  put(P->ctype.data(), sizeof(int) * (n + 1));
  put(P->rtype.data(), sizeof(int) * (m + 1));
  put(P->valid ? P->bvar.data() : nullptr, sizeof(int) * (m + 1));
  put(P->valid ? P->nvar.data() : nullptr, sizeof(int) * (n + 1));
  put(P->valid ? P->nflag.data() : nullptr, sizeof(int) * (n + 1));
  b = b0 + align_up((size_t)(b - b0), 8);
  put(P->clb.data(), 8 * (size_t)(n + 1));
  put(P->cub.data(), 8 * (size_t)(n + 1));
  put(P->rlb.data(), 8 * (size_t)(m + 1));
  put(P->rub.data(), 8 * (size_t)(m + 1));
  for (int i = m_base + 1; i <= m; i++) put(P->A[(size_t)i]->data(), 8 * (size_t)(n + 1));
  unsigned char *d = (unsigned char *)dev_buf;
  HIPCHECK(hipMemcpyAsync(d, host.data(), hb, hipMemcpyHostToDevice, sc.stream));
  if (P->valid) {
    SlabLayout L = slab_layout(P->m_cap, P->ld);
    const size_t tb = (size_t)(m + 1) * P->ld * 8;
    HIPCHECK(hipMemcpyAsync(d + hb, P->d_T, tb, hipMemcpyDeviceToDevice, sc.stream));
    HIPCHECK(hipMemcpyAsync(d + hb + align_up(tb, 256), (const unsigned char *)P->slab + L.o_bvar, L.total - L.o_bvar,
                            hipMemcpyDeviceToDevice, sc.stream));
  }
  HIPCHECK(hipStreamSynchronize(sc.stream));
  return 0;
}

// buffers for node images (mvx_image_api): plain device allocations on the bound device
void *engine_image_alloc(size_t bytes) {
  Context &c = ctx();
  if (hipSetDevice(c.dev) != hipSuccess) return nullptr;
  void *p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void engine_image_free(void *p) {
  if (p) (void)hipFree(p);
}

// dst already holds a copy of the receiver's root MODEL (rows 1..m_base, objective, kinds); the appended rows,
// bounds, basis and tableau come from the image
int engine_unpack(mvx_prob *dst, const void *dev_buf) {
  Context &c = ctx();
  MAIN_LOCK(c);
  flush_copies(c);
  SolveCtx &sc = c.main;
  const unsigned char *d = (const unsigned char *)dev_buf;
  PackHdr h;
  HIPCHECK(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, sc.stream));
  HIPCHECK(hipStreamSynchronize(sc.stream));
  if (h.magic != PACK_MAGIC || h.m_base != dst->m || h.n != dst->n || h.m < h.m_base) return -1;
  const int m = (int)h.m, n = (int)h.n, m_base = (int)h.m_base;
  std::vector<unsigned char> host((size_t)h.host_bytes);
  HIPCHECK(hipMemcpyAsync(host.data(), d, (size_t)h.host_bytes, hipMemcpyDeviceToHost, sc.stream));
  HIPCHECK(hipStreamSynchronize(sc.stream));
  const unsigned char *b = host.data() + sizeof(PackHdr);
  const unsigned char *b0 = b;
  auto get = [&](void *dstp, size_t bytes) {
    if (dstp) std::memcpy(dstp, b, bytes);
    b += bytes;
  };
  dst->m = m;
  dst->A.resize((size_t)m + 1);
  dst->rtype.resize((size_t)m + 1);
  dst->rlb.resize((size_t)m + 1);
  dst->rub.resize((size_t)m + 1);
  get(dst->ctype.data(), sizeof(int) * (n + 1));
  get(dst->rtype.data(), sizeof(int) * (m + 1));
  if (h.valid) {
    dst->bvar.assign((size_t)m + 1, 0);
    dst->nvar.assign((size_t)n + 1, 0);
    dst->nflag.assign((size_t)n + 1, 0);
  }
  get(h.valid ? dst->bvar.data() : nullptr, sizeof(int) * (m + 1));
  get(h.valid ? dst->nvar.data() : nullptr, sizeof(int) * (n + 1));
  get(h.valid ? dst->nflag.data() : nullptr, sizeof(int) * (n + 1));
  b = b0 + align_up((size_t)(b - b0), 8);
  get(dst->clb.data(), 8 * (size_t)(n + 1));
  get(dst->cub.data(), 8 * (size_t)(n + 1));
  get(dst->rlb.data(), 8 * (size_t)(m + 1));
  get(dst->rub.data(), 8 * (size_t)(m + 1));
  for (int i = m_base + 1; i <= m; i++) {
    auto row = std::make_shared<std::vector<double>>((size_t)n + 1, 0.0);
    get(row->data(), 8 * (size_t)(n + 1));
    dst->A.set((size_t)i, row);
  }
  dst->status = (int)h.status;
  dst->it_cnt = (int)h.it_cnt;
  dst->hint_dual = h.hint_dual != 0;
  dst->piv_since_check = (int)h.reserved;
  std::memcpy(dst->last_tol, h.last_tol, sizeof(dst->last_tol));
  dst->sol_fresh = false;
  dst->fresh_rows = -1;
  release_device(dst);
  dst->pending.clear();
  dst->valid = false;
  if (h.valid) {
    SlabLayout L = slab_layout((int)h.m_cap, (int)h.ld);
    void *slab = slab_alloc(c, L.total);
    if (!slab) return -2;
    bind_slab(dst, slab, (int)h.m_cap, (int)h.ld);
    const size_t tb = (size_t)(m + 1) * dst->ld * 8;
    HIPCHECK(hipMemcpyAsync(dst->d_T, d + h.host_bytes, tb, hipMemcpyDeviceToDevice, sc.stream));
    HIPCHECK(hipMemcpyAsync((unsigned char *)slab + L.o_bvar, d + h.host_bytes + align_up(tb, 256), L.total - L.o_bvar,
                            hipMemcpyDeviceToDevice, sc.stream));
    HIPCHECK(hipStreamSynchronize(sc.stream));
    rebuild_pos(dst);
    dst->valid = true;
  }
  return 0;
}

void tuning(int tr, int hot, int nt) {
  sync_stream();
  set_tuning(tr, hot, nt);
  if (g_ctx) { // partial-buffer sizes depend on the row-block depth
    g_ctx->main.sc_m_cap = 0;
    g_ctx->main.sc_ld = 0;
  }
}

void set_dual_chain(int len) { g_dchain = (len <= 0) ? 0 : std::min(DCH_MAX, len); } // <= 0: by batch width / size
void set_dual_fused(int mode) { g_dual_fused.store(mode < 0 ? -1 : (mode > 2 ? 2 : mode)); } // -1: MVX_DUAL_FUSED if set, else the size rule
void dual_fused_stats(long long *boots, long long *pivots) {
  *boots = g_dfused_boots.load();
  *pivots = g_dfused_pivots.load();
}
void set_chain(int len) { g_chain = (len <= 0) ? 0 : std::min(KCH, len); } // 0: by tableau size
void set_cluster(int on) { // 0: k_pc / k_pr per step; 1: k_chain (default); also forgets an earlier abort
  g_cluster.store(on != 0);
  g_cluster_broken.store(false);
}
void cluster_stats(long long *launches, long long *aborts) {
  *launches = g_cluster_launches.load();
  *aborts = g_cluster_aborts.load();
}
void set_persist(int mode) {
  g_persist_mode = mode < 0 ? -1 : (mode > 2 ? 2 : mode); // 2: no size cap
  g_persist_broken = false;
}
void persist_stats(long long *launches, long long *aborts) {
  *launches = g_persist_launches;
  *aborts = g_persist_aborts;
}
// cycle totals of workgroup 0 per phase since the context was created: propose, gather, read, apply, pivots
void persist_cycles(unsigned long long *out5) {
  for (int k = 0; k < 48; k++) out5[k] = 0;
  if (!g_ctx || !g_ctx->main.h_pabort) return;
  const unsigned long long *d = (const unsigned long long *)(g_ctx->main.h_pabort + 16);
  for (int k = 0; k < 48; k++) out5[k] = d[k];
}
// diagnostic (MVX_FCS_DBG=1): the last phase stamps of k_pc / k_pr (8 each) or k_chain per chain position, 10 ns ticks
int fcs_debug_stamps(unsigned long long *out) {
  Context &c = ctx();
  if (!c.main.h_ctl || !c.main.h_ctl->dbg) return 0;
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(out, c.main.h_ctl->dbg, (size_t)KCH * 16 * 8, hipMemcpyDeviceToHost));
  return KCH;
}
void set_stall_limit(int limit) { g_stall_limit = limit > 0 ? limit : 0; }
void set_batch_slots(int k) { g_batch_slots = k < 2 ? 2 : (k > 256 ? 256 : k); }
void profile_enable(int on) { ctx().prof = on != 0; }
void profile_reset() {
  Context &c = ctx();
  MAIN_LOCK(c);
  c.prof_update_ms = 0.0;
  c.prof_update_n = 0;
}
double profile_update_ms() { return g_ctx ? g_ctx->prof_update_ms : 0.0; }
long long profile_update_launches() { return g_ctx ? g_ctx->prof_update_n : 0; }

} // namespace mvx
