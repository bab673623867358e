// bayesnmf_amd/csrc/api.hip — C ABI of libbnmf.so (include/bnmf.h) over the gfx950 kernels.
// Host side: device memory, three HIP streams per handle, the constructor draws (R/bayesNMF_sampler.R:232-257).  The launch sequencing of
// the sweep (:273-285) is in sweep.h, the allocation kernels' static schedules in zplan.h, the posterior calls on a recorded range in
// posterior.h, the state file in state_io.h: all four are included here (one translation unit).  There is no CPU path.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cerrno>
#include <algorithm>
#include <map>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>
#include "kernels.h"
#include "zalloc_reg.h"
#include "zalloc_sort.h"
#include "zalloc_tile.h"
#include "zalloc_step.h"
#include "rank.h"
#include "mh.h"
#include "waic.h"
#include "ppc.h"
#include "attribution.h"
#include "mixing.h"
#include "relabel.h"
#include "project.h"
#include "decompose.h"
#include "contrast.h"
#include "regress.h"
#include "coactivity.h"
#include "stability.h"
#include "reconstruction.h"
#include "similarity.h"
#include "subtypes.h"
#include "residuals.h"
#include "tradeoff.h"
#include "prune.h"
#include "summary.h"

using namespace bnmf;

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return code;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(BNMF_EHIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

enum { KN_PDRAW = 0, KN_EDRAW = 1, KN_ZALLOC = 2, KN_REDUCE = 3, KN_SIDE = 4, KN_RANK = 5, KN_MH = 6, KN_OTHER = 7 };
static const char* k_names[BNMF_NKERNEL] = {"k_pdraw", "k_edraw", "k_zalloc", "k_reduce", "k_side", "k_rank", "k_mh", "other"};

// ---- device memory of the handles: a small per-device pool ----
// bnmf_destroy followed by bnmf_create (bayesNMF() after bayesNMF(), a BIC sweep, the fuzzers) freed ~60 device allocations and made them
// again.  The re-made allocations cost the next handle a wait of 8-13 ms (rounds 3-4; 27 ms with round 5's Mhat buffers: about a
// millisecond per MB) at its first synchronisation — the driver remaps freed memory lazily, at the first submission that touches it; a
// first handle of a process never saw it (tools/recreate.py: the wait sat in the first bnmf_set_array's stream synchronisation, lives
// 1, 2, 3 of a process, not life 0).  Freed blocks now go to a per-device free list keyed by their size and the next handle of the same
// shape takes them from there: no free, no map, no wait.  Blocks above 256 MB (the record_sample rings: their own cache below) and
// whatever exceeds BNMF_POOL_GB (default 1) are really freed; bnmf_trim() empties the list; an allocation that fails empties it and
// is tried again.
struct DevPool {
  std::mutex m;
  std::multimap<size_t, void*> free_blocks;
  std::map<void*, size_t> live;
  size_t cached = 0;
};
static DevPool g_pool[64];
static size_t pool_cap() { static const size_t cap = [] { const char* e = getenv("BNMF_POOL_GB"); return (size_t)((e ? atof(e) : 1.0) * 1e9); }(); return cap; }
static size_t pool_drop(int device) {
  if (device < 0 || device >= 64) return 0;
  std::vector<void*> drop;
  size_t tot = 0;
  { std::lock_guard<std::mutex> lk(g_pool[device].m); for (auto& kv : g_pool[device].free_blocks) drop.push_back(kv.second); tot = g_pool[device].cached; g_pool[device].free_blocks.clear(); g_pool[device].cached = 0; }
  for (void* q : drop) (void)hipFree(q);
  return tot;
}
static hipError_t dmalloc_raw(void** out, size_t bytes) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || bytes == 0 || bytes > ((size_t)256 << 20)) return hipMalloc(out, bytes);
  DevPool& P = g_pool[dev];
  {
    std::lock_guard<std::mutex> lk(P.m);
    auto it = P.free_blocks.find(bytes);
    if (it != P.free_blocks.end()) { *out = it->second; P.free_blocks.erase(it); P.cached -= bytes; P.live[*out] = bytes; return hipSuccess; }
  }
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); pool_drop(dev); e = hipMalloc(out, bytes); }
  if (e == hipSuccess) { std::lock_guard<std::mutex> lk(P.m); P.live[*out] = bytes; }
  return e;
}
template <class T> static hipError_t dmalloc(T** out, size_t bytes) { return dmalloc_raw((void**)out, bytes); }
static hipError_t dfree(void* p) {
  if (!p) return hipSuccess;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipFree(p);
  DevPool& P = g_pool[dev];
  {
    std::lock_guard<std::mutex> lk(P.m);
    auto it = P.live.find(p);
    if (it != P.live.end()) {
      const size_t bytes = it->second;
      P.live.erase(it);
      if (P.cached + bytes <= pool_cap()) { P.free_blocks.insert({bytes, p}); P.cached += bytes; return hipSuccess; }
    }
  }
  return hipFree(p);
}


#include "zplan.h"   // Switches and the planners of bnmf_create (device-free)

struct Arr { double* d = nullptr; size_t n = 0; int stride = 1; bool set = false; std::vector<int> redraw; double* ring = nullptr;
             bool slab = false; };   // slab: d points into the handle's block of scalars (a broadcast hyper-prior value), not an allocation of its own

// What one sweep hands to the next: the host's record of what is in flight on the three streams (sweep.h is its only writer
// apart from the two resets below).  Configuration chosen at bnmf_create (mh.pipe, mh.side_main, gate_forced, serial, dbg_*) is
// not in here.  The default member initialisers ARE the reset values: a chain starts (bnmf_init on a used handle, bnmf_load_state)
// with `pipe = Pipe{}` behind drained streams and cleared sync words.  "t" below is the iteration a sweep is about to run.
//
// The hyper sweep of t (prior parameters, Esum; issued during t - 1)
//   side_valid     it has been issued.  Set by every launch_side* (launch_side_early only with its launch_side_late), by k_mh_tail / the
//                  hosted MH sweep when they carry it; read at the top of every sweep, which issues it by launch_side if not.
//   side_main      ... on the main stream (launch_side_main, k_mh_tail, the hosted MH sweep): the draws of t need neither poll nor wait.
//                  MH / Normal sweeps only.  side_main implies side_valid and !flags_valid.
//   flags_valid    ... by kernels that publish flags [1] (E side) and [3] (Esum) = t, which the draw kernels may poll instead of a stream
//                  wait.  Read as `poll = flags_valid && !profile && !serial`; meaningful only while side_valid (bnmf_set_array
//                  leaves it, the launch_side that follows clears it).
//   side_ev_stale  ev_sideP / ev_side have not been recorded behind it.  True only after launch_side_E / launch_side_merged (the fixed-rank
//                  Gibbs sweep, where nobody waits for them in the steady state); whoever needs the events calls refresh_side_events.
//   gate_f0        the flag that says its E side (merged path: its P side) is done, beside [3]: 9 after launch_side_merged (P side on `side`
//                  under [9], E side inside k_draw), 1 after a split sweep's k_pdraw.  Read by the allocation kernel's gate (zargs) and by the
//                  split sweep that follows a merged one.  Never 9 when the rank is learned.
// The allocation kernel's gate (merged draw path)
//   z_gate_next    != 0 only inside sweep(), around launch_zalloc: the kernel being launched waits at its end for the hyper sweep of this
//                  iteration (t + 1).  Set and cleared by sweep(), read by zargs.
//   z_gated_for    what z_gate_next was for the last allocation kernel.  z_gated_for == t only if the allocation kernel of t - 1 was launched
//                  with a gate: then k_draw of t may start without a poll of its own.  Read by sweep()'s choice only, and only under poll.
// Reductions issued late (all three are empty between two API calls: bnmf_init and run_impl flush them at their ends)
//   red_pending, red_t, red_row   k_reduce of iteration red_t into metric row red_row has not been issued (launch_reduce); taken by the next
//                  sweep's side launches (issue_pending_reduce), by the MH tail kernels as workgroups (take_reduce_slots), or by flush_reduce.
//   red_issued     ev_red has been recorded at least once (a k_reduce off side2): side2's log-prior kernels wait for it (lpPn slot reuse).
//   red_on_side2   the last k_reduce went to side2 itself: stream order, no wait for ev_red.
//   ct_pending     iteration whose column terms (sorted schedule) have not been summed; taken by take_colterms / flush_colterms.
//   mh_etail_pending   hosted MH sweep: iteration whose E side has not been issued; taken by the next row sweep or flush_mh_etail.
// Buffers a sweep leaves prepared for the next
//   mh_prep_valid  MH / Normal sweeps: Et, nzE are current and nzP is zero (k_mh_tail of the previous iteration).
//   mh_pipe_valid  hosted MH sweep: its Et / parity flag buffers are current.  At most one of the two is true: launch_mh_PE prepares the
//                  form it runs and invalidates the other.
//   z_expanded_iter   save_Z on the sorted schedule: the iteration whose Z is in dZ, expanded from its records (ensure_Z).
struct Pipe {
  bool side_valid = false, side_main = false, flags_valid = false, side_ev_stale = false;
  int gate_f0 = 1;
  uint32_t z_gate_next = 0, z_gated_for = 0;
  bool red_pending = false, red_issued = false, red_on_side2 = false; uint32_t red_t = 0; int red_row = 0;
  uint32_t ct_pending = 0, mh_etail_pending = 0;
  bool mh_prep_valid = false, mh_pipe_valid = false;
  int z_expanded_iter = 0;
  // bnmf_set_array (streams drained, the chain goes on): the hyper sweep of iter + 1 and the MH sweeps' prepared buffers were made from
  // the value just replaced.  Narrower than a reset, and enough: the next sweep finds !side_valid and calls launch_side, which
  // clears flags_valid, side_main and side_ev_stale and records ev_side; hence poll is false in that sweep, the main stream waits for
  // ev_side, and what survives is not read before it is rewritten — gate_f0 and z_gated_for are read only under poll (the allocation kernel
  // is gated only under poll, too), z_gated_for is written by every sweep and gate_f0 by every sweep that leaves flags_valid set; red_issued only says that ev_red may be waited for, which stays true.
  // A full reset would also change that first sweep's runtime calls (no wait for ev_red).
  void invalidate_prepared() { side_valid = false; side_main = false; mh_prep_valid = false; mh_pipe_valid = false; }
};

// Which allocation kernel a Poisson handle launches: chosen once, by create_zalloc, in this order — step before tile before the sorted
// schedule, else the wave-per-column kernel that fits.  launch_zalloc switches on it.  `reg` and `sort` are the two kinds for which
// the register kernel was eligible (N <= 24 and its LDS fits): what the merged draw kernel asks (merged_draw_ok).  Modifiers, not
// kinds: ZTile::lean (tile) and, in -DBNMF_DIAG builds, z_ablate (reg: the sorted schedule is then not tried).
enum class ZKind { none /* Normal: counts are not allocated */, general /* k_zalloc */, reg /* k_zalloc_reg */, tile, step, sort };

// What bnmf_create decides and acquires for one kernel family, each with its device buffers.  All of them: written by bnmf_create only
// (create_rank, create_mh, create_zalloc, build_zsort, build_zstep below) unless a member says otherwise; a group whose kernel the
// handle does not launch stays at its defaults (null pointers).  The planners' halves are in zplan.h.
// The wave-per-column kernels (ZKind::reg, ::general) need no buffers of their own: ZWavePlan zw is the whole group; read by launch_z.
// k_zalloc_tile (ZKind::tile); read by launch_ztile.  g.dbg (BNMF_ZTDBG) is a device buffer too.
struct ZTile : ZTilePlan { double* dMhat = nullptr; };
// k_zalloc_sort (ZKind::sort: stats mode, N <= 24) — the static schedule built from M; read by launch_zsort, launch_zexpand, ensure_Z,
// zs_rec_at, the column terms (colterms.h launches in sweep.h), bnmf_get_stat and state_io.h (records).
struct ZSort {
  bool pk = false, shared = false;     // two factors per word; large cells spread over the blocks: ZsumK is accumulated (atomics), the draw kernels zero it
  ZSGeom g{}; int nblk = 0, w = 0; size_t lds = 0;
  int it16 = 0, qmax = ZS_QMAX;        // 2-byte items; quads per item
  int fixed = 0;                       // the geometry-fixed instantiation the schedule fits (zsort_fixed_form; 0: none, or BNMF_ZSFIXED=0)
  int nempty = 0;                      // blocks without an own column (bnmf_get_stat 7)
  uint32_t* dItems = nullptr; ZSBlock* dBlocks = nullptr; int* dCols = nullptr; int32_t* dM = nullptr; unsigned long long* dProf = nullptr;
  double* dMh = nullptr;               // [3][G][K] Mhat left by k_zalloc_sort for the per-column metric terms (colterms.h)
  // save_Z: Z is kept AS RECORDS (two 16-bit counts per word and item: 44 MB per iteration at the metric configuration against 77 MB of Z)
  // and expanded when somebody reads it (bnmf_get_array, bnmf_window).  With a window the records of iteration t live in slot
  // (t - 1) % wcap of dRecRing (samples$Z; made by ensure_rings at bnmf_init); eager (BNMF_ZEAGER=1, measurements): expand every iteration.
  uint32_t *dRec = nullptr, *dRecRing = nullptr; size_t recwords = 0; bool eager = false;
  int x_cols = 0; size_t x_lds = 0;    // k_zexpand's columns per pass and LDS bytes
};
// k_zalloc_step (ZKind::step: stats mode, 25 <= N <= 100, any K) — the static schedule built from M; read by launch_zstep, bnmf_get_stat.
struct ZStep {
  ZPGeom g{}; int ns = 0 /* waves per workgroup */, gbp = 0; size_t lds = 0; bool it16 = false;
  uint32_t* dItems = nullptr; ZPWg* dWgs = nullptr; ZPBatch* dBatches = nullptr; ZPStep* dSteps = nullptr; int* dCols = nullptr;
};
// The rank sweep (learning_rank); read by launch_rank, bnmf_debug_rank; dSync / dCol are cleared where a chain starts.
struct Rank : RankPlan { double *dCol = nullptr, *dMhat = nullptr; uint32_t* dSync = nullptr; void* dDbg = nullptr; };
// The MH / Normal sweeps; read by sweep_mh / sweep_mh_pipe and their launch helpers (sweep.h), refresh_dev, bnmf_get_stat.
struct Mh : MhPlan {
  bool side_tail = true;               // BNMF_MHSIDETAIL=0 (diagnostics): the main-stream hyper sweep as a launch of its own in front of k_mh_tail
  bool side_main = true;               // BNMF_MHSIDE=0 (diagnostics / tests): the hyper sweep on the side stream, as in round 3
  bool no_reg = false;                 // BNMF_MHREG=0 (tests): the row sweep in the form that keeps Mhat in memory also where its register form fits
  bool e_k128 = false;                 // BNMF_MHE_K128=1 (diagnostics / tests): k_mh_ecol16's 128-row form also where K <= 96
  int e_gw = 0;                        // BNMF_MHE_GW: lanes per column of k_mh_ecol16 (0 = by mode)
  double *dMhat = nullptr, *dAccPn = nullptr, *dAccEpart = nullptr, *dEt = nullptr; int* dNzE = nullptr;
  int32_t* dMt = nullptr; double* dMtf = nullptr;   // the [G][K] transpose of the data: counts, or fp64 on a Normal handle
};

struct Scratch { unsigned char* p = nullptr; size_t bytes = 0; };   // a device block and its size (scratch_reserve, posterior.h)

struct bnmf_handle {
  bnmf_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;        // main stream: draws, k_zalloc, reductions
  hipStream_t side = nullptr;          // side stream: k_side (E part) of the next iteration (overlaps k_zalloc), k_reduce
  hipStream_t side2 = nullptr;         // second side stream: k_side P part (starts right after k_pdraw) and Esum
  hipEvent_t ev_draw = nullptr, ev_side = nullptr, ev_sideP = nullptr, ev_p = nullptr, ev_z = nullptr, ev_red = nullptr, ev_rank = nullptr;
  // Every pooled device block made for the handle (hmalloc), in the order made: bnmf_destroy frees the list, hfree takes a block out
  // early (one grown on demand that is being replaced).  Not in here, released by name in bnmf_destroy: Arr::d and Arr::ring, the three
  // hipHostMalloc blocks (hMetrics, hErr, hStage), events, streams, the lock files.
  std::vector<void*> owned;
  int gate_forced = -1;                // BNMF_GATE at bnmf_create: 0 / 1 forces the merged draw kernel off / on, else by size
  int draw_bw = 0;                     // lanes per workgroup of the merged draw kernel (chosen at the first launch)
  double* dScal = nullptr;              // [BNMF_ID_MAX] broadcast scalars of bnmf_set_array (hyper-prior values given as one number)
  unsigned* dDrawOwn = nullptr; unsigned draw_seq = 0;   // k_draw: owner word per column of P, launch sequence number (kernels.h).  draw_seq is NOT part of
                                       // Pipe: it only has to differ from launch to launch, so bnmf_init leaves it running; bnmf_load_state zeroes it with dDrawOwn
  bool draw_fixed_ok = true;           // BNMF_DRAWFIXED (read at bnmf_create): 0 = k_draw always in its dynamic form (sweep.h draw_fixed_form)
  int dbg_draw_no_p = 0;               // BNMF_DEBUG_DRAW_NO_P (tests): the P workgroups of k_draw leave without claiming their columns
  int dbg_main_delay_us = 0;           // BNMF_DEBUG_MAIN_DELAY_US (tests): a delay kernel in front of the main stream's kernels of every sweep
  int dbg_allside_delay_us = 0;        // BNMF_DEBUG_ALLSIDE_DELAY_US (tests): a delay kernel in front of EVERY kernel launched on the two side streams
  int dbg_side_delay_us = 0;           // BNMF_DEBUG_SIDE_DELAY_US (tests): a delay kernel in front of the P-side hyper sweep of launch_side_merged
  double* E_alt = nullptr;             // Gibbs sweep: the other E buffer (k_edraw of t+1 does not overwrite what k_lpe of t still reads)
  const void* z_attr_kernel = nullptr;   // allocation kernel whose dynamic-LDS limit has been raised for this handle (raise_lds_limit, sweep.h)
  Pipe pipe;                           // what one sweep hands to the next (above); reset where a chain starts: bnmf_init, bnmf_load_state
  int iter = 0;
  bool inited = false;
  Dev dev{};
  Arr arr[BNMF_ID_MAX];
  int32_t *dM = nullptr, *dZsumK = nullptr, *dZsumG = nullptr, *dZ = nullptr;
  double* dMf = nullptr;               // Normal handles: the data as fp64, M's layout (dM stays unset)
  int* dR = nullptr; int* dRedraw = nullptr;
  std::vector<int32_t> fixedP;         // bnmf_set_fixed: 1 = column n of P is held at its value (empty: never called); n_fixed of them are;
  int n_fixed = 0; int* dFixedP = nullptr;   // dFixedP [N]: the mask the kernels read (Dev::fixedP; null there while no column is fixed)
  double *dEsum = nullptr, *dPsum = nullptr, *dlpPn = nullptr, *dlpE = nullptr, *dcol = nullptr;
  double* hMetrics = nullptr;          // the metric rows live in mapped host memory (dMetrics is its device address): k_compose writes them
                                       // where the host reads them, no device-to-host copy at the end of a call
  double *dLut = nullptr, *dTemp = nullptr, *dMetrics = nullptr, *dRaw = nullptr;
  int32_t* zring = nullptr;            // save_Z with a window: samples$Z, [wcap][K*N*G] int32 (only if it fits BNMF_ZRING_GB, default 32)
  size_t metrics_rows = 0;
  int maxM = 0, nblkE = 0;
  long colmax = 0;                     // largest column total of M (Poisson)
  int n_cu = 256;
  int wcap = 0;                        // ring capacity = window + 1: the hyper sweep of iteration t+1 is issued (and, in the
                                       // Gibbs sweep, recorded) during iteration t, one slot ahead of the oldest kept sample
  ZKind zkind = ZKind::none;           // the allocation kernel (above), and the groups of bnmf_create's choices
  int z_ablate = 0;
  ZWavePlan zw; ZTile zt; ZSort zs; ZStep zp; Rank rank; Mh mh;
  hipEvent_t ev[2 * BNMF_NKERNEL]{};
  bool have_ev = false;
  Scratch scratch;                     // of the posterior calls (posterior.h): grown on demand, carved by one call at a time, nothing in it outlives a call
  int devlock_fd = -1;                 // the device's lock file (<BNMF_LOCKDIR or /tmp>/bnmf_dev_<PCI bus id>.lock): the device gate's rule across the PROCESSES that share the device
  int devgate_fd = -1;                 // ... and its turnstile (.gate): a process that wants the device exclusively holds it while it waits, new sharers queue behind it
  bool devlock_off = false;            // BNMF_DEVLOCK=0: the caller vouches that no other process uses the device
  unsigned* dFlags = nullptr;                     // [0] counter, [1] flag of the E-side hyper sweep; [2], [3] of P part + Esum; [5], [6] P inside k_draw;
                                                  // [8], [9] P-side sweep on its own stream
  int* hErr = nullptr; int* dErr = nullptr;       // time-out words of the bounded in-kernel waits, in mapped host memory (read without a copy):
                                                  // [0] a draw kernel waiting for the hyper sweep, [1] the rank sweep's exchange
  bool serial = false;                            // no kernel may wait for a kernel of another stream (serialised dispatch: counter
                                                  // collection, AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING; or BNMF_SERIAL=1): stream waits only
  bool poisoned = false;                          // a bounded in-kernel wait timed out: the state is no longer the chain's, every call fails
  std::vector<double> hist;                       // [wcap][4]: loglikelihood, logposterior, P / E mean acceptance of the last iterations
  std::vector<double> temp_host;                  // temperature schedule (host copy, for the convergence rule)
  uint64_t data_hash = 0;                         // hash of the data as the handle holds it (int32 counts, fp64 for Normal): bnmf_save_state's file header
  unsigned char* hStage = nullptr;                // two pinned halves of bnmf_save_state / bnmf_load_state (state_io.h), made at the first of them
};

// The one owner of a handle's pooled device memory: make a block and register it; make it zeroed; make it and fill it from the host.
template <class T> static hipError_t hmalloc(bnmf_handle* h, T** out, size_t bytes) {
  const hipError_t e = dmalloc(out, bytes);
  if (e == hipSuccess) h->owned.push_back(*out);
  return e;
}
template <class T> static hipError_t hzeroed(bnmf_handle* h, T** out, size_t bytes) {
  const hipError_t e = hmalloc(h, out, bytes);
  return e != hipSuccess ? e : hipMemset(*out, 0, bytes);
}
template <class T> static hipError_t hupload(bnmf_handle* h, T** out, const void* src, size_t bytes, size_t alloc_bytes = 0) {
  const hipError_t e = hmalloc(h, out, alloc_bytes ? alloc_bytes : bytes);
  return e != hipSuccess ? e : hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice);
}
// ... and give one up before the handle goes (a buffer grown on demand, about to be replaced by a larger one)
template <class T> static hipError_t hfree(bnmf_handle* h, T*& p) {
  if (!p) return hipSuccess;
  h->owned.erase(std::remove(h->owned.begin(), h->owned.end(), (void*)p), h->owned.end());
  const hipError_t e = dfree(p);
  p = nullptr;
  return e;
}

static size_t id_len(const bnmf_handle* h, int id) {
  const size_t K = h->cfg.K, G = h->cfg.G, N = h->cfg.N;
  switch (id) {
    case BNMF_P: case BNMF_ZSUMG: case BNMF_ALPHA_P: case BNMF_BETA_P: case BNMF_MU_P: case BNMF_SIGMASQ_P:
    case BNMF_LAMBDA_P: case BNMF_HA_P: case BNMF_HB_P: case BNMF_HC_P: case BNMF_HD_P: case BNMF_HM_P:
    case BNMF_HS_P: case BNMF_ACC_P: return K * N;
    case BNMF_E: case BNMF_ZSUMK: case BNMF_ALPHA_E: case BNMF_BETA_E: case BNMF_MU_E: case BNMF_SIGMASQ_E:
    case BNMF_LAMBDA_E: case BNMF_HA_E: case BNMF_HB_E: case BNMF_HC_E: case BNMF_HD_E: case BNMF_HM_E:
    case BNMF_HS_E: case BNMF_ACC_E: return N * G;
    case BNMF_A: return N;
    case BNMF_R: return 1;
    case BNMF_Z: return K * N * G;
    case BNMF_SIGMASQ: case BNMF_ALPHA: case BNMF_BETA: return G;
    case BNMF_MHAT: return K * G;
    default: return 0;
  }
}
static bool is_hyper(int id) { return (id >= 30 && id < 50) || id == BNMF_ALPHA || id == BNMF_BETA; }
static bool is_prior_param(int id) { return id >= BNMF_ALPHA_P && id <= BNMF_LAMBDA_E; }   // 2 slots, slot(t) = t & 1
static int cur_slot(const bnmf_handle* h) { return (h->iter > 0 ? h->iter : 1) & 1; }
static bool is_pside(int id) { return id == BNMF_P || id == BNMF_ALPHA_P || id == BNMF_BETA_P || id == BNMF_MU_P || id == BNMF_SIGMASQ_P || id == BNMF_LAMBDA_P; }

static int ensure_Z(bnmf_handle* h);   // save_Z on the sorted schedule: Z of the current iteration expanded from its records, if it is not
static int ensure(bnmf_handle* h, int id) {
  Arr& a = h->arr[id];
  if (a.d) return 0;
  const size_t n = id_len(h, id), tot = n * (is_prior_param(id) ? 2 : 1);
  HIPCHK(dmalloc(&a.d, tot * sizeof(double)));
  std::vector<double> nan(tot, std::nan(""));
  HIPCHK(hipMemcpy(a.d, nan.data(), tot * sizeof(double), hipMemcpyHostToDevice));
  a.n = n; a.stride = 1;
  return 0;
}

static void refresh_dev(bnmf_handle* h) {
  Dev& d = h->dev;
  const bnmf_config& c = h->cfg;
  d.K = c.K; d.G = c.G; d.N = c.N;
  d.prior = c.prior; d.likelihood = c.likelihood; d.MH = c.MH; d.learning_rank = c.learning_rank;
  d.rank_method = c.rank_method; d.save_Z = c.save_Z;
  d.zsumk_accum = (h->zkind == ZKind::tile || (h->zkind == ZKind::sort && h->zs.shared)) ? 1 : 0;
  d.k0 = (uint32_t)c.seed; d.k1 = (uint32_t)(c.seed >> 32) ^ c.chain_id;
  d.maxM = h->maxM;
  d.M = h->dM; d.Mt = h->mh.dMt; d.Mf = h->dMf; d.Mtf = h->mh.dMtf; d.Et = h->mh.dEt; d.R = h->dR;
  d.P = h->arr[BNMF_P].d; d.E = h->arr[BNMF_E].d; d.A = h->arr[BNMF_A].d;
  d.ZsumK = h->dZsumK; d.ZsumG = h->dZsumG; d.Z = h->dZ;
  d.Alpha_p = h->arr[BNMF_ALPHA_P].d; d.Beta_p = h->arr[BNMF_BETA_P].d;
  d.Alpha_e = h->arr[BNMF_ALPHA_E].d; d.Beta_e = h->arr[BNMF_BETA_E].d;
  d.Mu_p = h->arr[BNMF_MU_P].d; d.Sig_p = h->arr[BNMF_SIGMASQ_P].d;
  d.Mu_e = h->arr[BNMF_MU_E].d; d.Sig_e = h->arr[BNMF_SIGMASQ_E].d;
  d.Lam_p = h->arr[BNMF_LAMBDA_P].d; d.Lam_e = h->arr[BNMF_LAMBDA_E].d;
  auto hr = [&](int id) { return HRef{h->arr[id].d, h->arr[id].stride}; };
  d.hA_p = hr(BNMF_HA_P); d.hB_p = hr(BNMF_HB_P); d.hC_p = hr(BNMF_HC_P); d.hD_p = hr(BNMF_HD_P);
  d.hM_p = hr(BNMF_HM_P); d.hS_p = hr(BNMF_HS_P);
  d.hA_e = hr(BNMF_HA_E); d.hB_e = hr(BNMF_HB_E); d.hC_e = hr(BNMF_HC_E); d.hD_e = hr(BNMF_HD_E);
  d.hM_e = hr(BNMF_HM_E); d.hS_e = hr(BNMF_HS_E);
  d.sigmasq = h->arr[BNMF_SIGMASQ].d; d.hAlphaS = hr(BNMF_ALPHA); d.hBetaS = hr(BNMF_BETA);
  d.Esum = h->dEsum; d.Psum = h->dPsum; d.lpPn = h->dlpPn; d.lpE_part = h->dlpE;
  d.colsse = h->dcol; d.colll = h->dcol + c.G; d.colkl = h->dcol + 2 * (size_t)c.G;
  d.lgfact = h->dLut; d.logm = h->dLut + (h->maxM + 1);
  d.temperature = h->dTemp; d.n_temperature = c.n_temperature;
  d.metrics = h->dMetrics; d.raw = h->dRaw;
  d.lenP = (size_t)c.K * c.N; d.lenE = (size_t)c.N * c.G;
  d.fixedP = h->n_fixed > 0 ? h->dFixedP : nullptr;
}

// BNMF_TIMING=1 (diagnostics): wall-clock marks of bnmf_create on stderr
static bool timing_on() { return env_set("BNMF_TIMING"); }
struct CreateClock {
  bool on = timing_on(); std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void mark(const char* what) { if (!on) return; const auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[bnmf_create] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t0).count()); t0 = t; }
};
__global__ void k_set_scalar(double* p, double v) { *p = v; }

extern "C" {

int bnmf_destroy(bnmf_handle* h);
int bnmf_version(void) { return BNMF_VERSION; }
const char* bnmf_last_error(void) { return g_err; }
const char* bnmf_kernel_name(int i) { return (i >= 0 && i < BNMF_NKERNEL) ? k_names[i] : ""; }

int bnmf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int bnmf_device_info(int device, char* buf, size_t buflen) {
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, device));
  snprintf(buf, buflen, "%s arch=%s CUs=%d clock=%dMHz mem=%.1fGiB lds/block=%zu",
           p.name, p.gcnArchName, p.multiProcessorCount, p.clockRate / 1000,
           (double)p.totalGlobalMem / (1024.0 * 1024.0 * 1024.0), (size_t)p.sharedMemPerBlock);
  return 0;
}

static int create_impl(const bnmf_config* cfg, const int32_t* M, const double* Mf, bnmf_handle* h);
// lgamma / digamma table of the Alpha sampler's tangent points (dsamplers.h g_alut): filled once per device
static int ensure_alut(int device) {
  static bool done[64] = {};
  static std::mutex mtx;                                  // bnmf_create may be called from several host threads (one chain each)
  if (device < 0 || device >= 64) return fail(BNMF_EINVAL, "device %d out of range", device);
  std::lock_guard<std::mutex> lock(mtx);
  if (done[device]) return 0;
  hipLaunchKernelGGL(k_alut_fill, dim3((ALUT_N + 255) / 256), dim3(256), 0, 0, 0);
  hipLaunchKernelGGL(k_alut_fill, dim3((ALUT_N + 255) / 256), dim3(256), 0, 0, 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  done[device] = true;
  return 0;
}

// what both entry points refuse before they look at the data
static int check_args(const char* who, const bnmf_config* cfg, const void* M, bnmf_handle** out) {
  if (!cfg || !M || !out) return fail(BNMF_EINVAL, "%s: null argument", who);
  if (cfg->K < 1 || cfg->G < 1 || cfg->N < 1) return fail(BNMF_EINVAL, "%s: dims must be positive", who);
  if (cfg->N > 1024) return fail(BNMF_EINVAL, "%s: N > 1024 unsupported", who);
  return 0;
}
// M: int32 counts (bnmf_create), Mf: fp64 data (bnmf_create_f64, Normal only); exactly one is given
static int create_handle(const bnmf_config* cfg, const int32_t* M, const double* Mf, bnmf_handle** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(BNMF_ENODEVICE, "bnmf_create: no HIP device visible (libbnmf has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(BNMF_ENODEVICE, "bnmf_create: device %d out of range (%d visible)", cfg->device, ndev);
  // model check: check_model R/bayesNMF_sampler.R:623-645
  if (cfg->likelihood == BNMF_NORMAL) {
    if (cfg->prior == BNMF_GAMMA) return fail(BNMF_EMODEL, "prior must be one of c('truncnormal','exponential') with `likelihood = 'normal'`");
  } else if (cfg->likelihood == BNMF_POISSON) {
    if (cfg->prior == BNMF_GAMMA && cfg->MH) return fail(BNMF_EMODEL, "gamma prior cannot be used in a MH-within-gibbs sampler");
    if (cfg->prior == BNMF_TRUNCNORMAL && !cfg->MH) return fail(BNMF_EMODEL, "truncnormal prior can only be used in a MH-within-gibbs sampler");
  } else return fail(BNMF_EMODEL, "likelihood must be one of normal, poisson");
  HIPCHK(hipSetDevice(cfg->device));
  if (int rc = ensure_alut(cfg->device)) return rc;
  bnmf_handle* h = new bnmf_handle();
  h->cfg = *cfg;
  h->device = cfg->device;
  if (int rc = create_impl(cfg, M, Mf, h)) {         // every failure path releases the handle and its device memory
    char keep[sizeof g_err]; memcpy(keep, g_err, sizeof keep);
    bnmf_destroy(h);
    memcpy(g_err, keep, sizeof keep);
    return rc;
  }
  *out = h;
  return 0;
}

int bnmf_create(const bnmf_config* cfg, const int32_t* M, bnmf_handle** out) {
  if (int rc = check_args("bnmf_create", cfg, M, out)) return rc;
  return create_handle(cfg, M, nullptr, out);
}

// Real-valued data.  Every cell is checked here, on the host, before any device call.  Normal: any finite value (the handle keeps
// them as fp64); Poisson: whole numbers in [0, 2^31 - 1] only, converted exactly, then bnmf_create.
int bnmf_create_f64(const bnmf_config* cfg, const double* M, bnmf_handle** out) {
  if (int rc = check_args("bnmf_create_f64", cfg, M, out)) return rc;
  const size_t K = cfg->K, G = cfg->G;
  if (cfg->likelihood == BNMF_NORMAL) {
    for (size_t g = 0; g < G; ++g)
      for (size_t k = 0; k < K; ++k)
        if (!std::isfinite(M[k + K * g])) return fail(BNMF_EINVAL, "bnmf_create_f64: M[%zu, %zu] = %g is not finite", k, g, M[k + K * g]);
    return create_handle(cfg, nullptr, M, out);
  }
  if (cfg->likelihood != BNMF_POISSON) return fail(BNMF_EMODEL, "likelihood must be one of normal, poisson");
  std::vector<int32_t> mi(K * G);
  for (size_t g = 0; g < G; ++g)
    for (size_t k = 0; k < K; ++k) {
      const double v = M[k + K * g];
      if (!(v >= 0.0 && v <= 2147483647.0 && v == std::floor(v)))      // (NaN fails the first test)
        return fail(BNMF_EINVAL, "bnmf_create_f64: non-integer count M[%zu, %zu] = %g (likelihood = poisson takes whole numbers in [0, 2^31 - 1])", k, g, v);
      mi[k + K * g] = (int32_t)v;
    }
  return bnmf_create(cfg, mi.data(), out);
}

// build_zsort uploads what plan_zsort (zplan.h) returns; reg_ok: the register kernel is eligible (plan_zwave)
static int build_zsort(bnmf_handle* h, const int32_t* M, bool reg_ok, const Switches& sw) {
  const bnmf_config& c = h->cfg;
  const size_t K = c.K, G = c.G, N = c.N;
  ZSort& z = h->zs;
  ZSortPlan p;
  if (int rc = plan_zsort(M, K, G, N, c.save_Z != 0, h->maxM, reg_ok, h->n_cu, sw, p)) return rc;
  if (!p.ok) return 0;
  if (p.it16) HIPCHK(hupload(h, &z.dItems, p.items16.data(), p.items16.size() * sizeof(uint16_t), (p.items16.size() * sizeof(uint16_t) + 3) & ~(size_t)3));
  else HIPCHK(hupload(h, &z.dItems, p.items.data(), p.items.size() * sizeof(uint32_t)));
  z.it16 = p.it16 ? 1 : 0; z.qmax = p.qmax;
  HIPCHK(hupload(h, &z.dBlocks, p.blocks.data(), p.blocks.size() * sizeof(ZSBlock)));
  HIPCHK(hupload(h, &z.dCols, p.cols.data(), p.cols.size() * sizeof(int)));
  HIPCHK(hupload(h, &z.dM, p.Mblk.data(), p.Mblk.size() * sizeof(int32_t)));
  // three copies, iteration t in copy t % 3 (as the per-column partial sums): the terms of t are summed beside the allocation kernel of t + 1
  // (k_side_lp of t + 2, stream side2), which is known to be over before the draw kernel of t + 3 starts — the allocation kernel of t + 2
  // has waited for the flag of the k_side_lp behind it on that stream
  HIPCHK(hzeroed(h, &z.dMh, 3 * K * G * sizeof(double)));
  if (c.save_Z) {
    const size_t hw = (N + 1) / 2;
    z.recwords = p.items.size() * hw;
    HIPCHK(hmalloc(h, &z.dRec, z.recwords * sizeof(uint32_t)));
    z.eager = sw.z_eager;
    const size_t lds_max = 160 * 1024;
    z.x_cols = std::max(1, std::min(p.GBc, zexpand_cols((int)K, (int)N, lds_max)));
    z.x_lds = ((size_t)z.x_cols * N * ((K + 1) / 2) * 4 + 15) & ~(size_t)15;
    if (z.x_lds > lds_max) return fail(BNMF_EINVAL, "bnmf_create: K = %zu, N = %zu: a column of Z does not fit the LDS of k_zexpand", K, N);
    HIPCHK(hipFuncSetAttribute((const void*)k_zexpand, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  }
  z.g = ZSGeom{p.KP, p.GBc, p.nb};
  z.shared = p.shared;                                     // columns with several writers of ZsumK: atomics + zeroing by the consumer (refresh_dev)
  z.nblk = p.nblk; z.w = p.W; z.pk = p.pk; z.nempty = p.nempty;
  z.fixed = sw.zs_fixed ? zsort_fixed_form((int)K, (int)N, p.KP, p.GBc, z.it16, p.qmax, p.W, p.nblk, p.pk, p.shared, c.save_Z != 0) : 0;
  z.lds = (zsort_shared_bytes((int)K, (int)N, p.KP, p.GBc, p.pk) + (size_t)p.W * zsort_wave_bytes(p.nblk, (int)N) + 15) & ~(size_t)15;
  h->zkind = ZKind::sort;
#ifdef ZSPROF
  HIPCHK(hzeroed(h, &z.dProf, (8 + 3 * 16 * 8) * sizeof(unsigned long long)));   // section ticks, then the stamps of three blocks' waves (-DZSPROF)
#endif
  return 0;
}

// ... and build_zstep what plan_zstep returns
static int build_zstep(bnmf_handle* h, const int32_t* M, const Switches& sw) {
  const bnmf_config& c = h->cfg;
  ZStep& z = h->zp;
  ZStepPlan p;
  if (int rc = plan_zstep(M, c.K, c.G, c.N, c.save_Z != 0, h->n_cu, sw, p)) return rc;
  if (!p.ok) return 0;
  z.it16 = p.it16;
  if (p.it16) HIPCHK(hupload(h, &z.dItems, p.items16.data(), p.items16.size() * sizeof(uint16_t), (p.items16.size() * sizeof(uint16_t) + 3) & ~(size_t)3));
  else HIPCHK(hupload(h, &z.dItems, p.items.data(), p.items.size() * sizeof(uint32_t)));
  HIPCHK(hupload(h, &z.dWgs, p.wgs.data(), p.wgs.size() * sizeof(ZPWg)));
  HIPCHK(hupload(h, &z.dBatches, p.batches.data(), p.batches.size() * sizeof(ZPBatch)));
  HIPCHK(hupload(h, &z.dSteps, p.steps.data(), p.steps.size() * sizeof(ZPStep)));
  HIPCHK(hupload(h, &z.dCols, p.cols.data(), p.cols.size() * sizeof(int)));
  z.g = ZPGeom{p.nch, p.nwg, nullptr};
#ifdef ZPPROF
  HIPCHK(hzeroed(h, &z.g.prof, 8 * sizeof(unsigned long long)));
#endif
  z.ns = p.W; z.gbp = p.GBP;
  z.lds = (zstep_shared_bytes((int)c.N, p.GBP) + p.W * zstep_wave_bytes(p.L) + 15) & ~(size_t)15;
  h->zkind = ZKind::step;
  return 0;
}

// A handle's three streams come from a per-device pool and go back to it at bnmf_destroy: creating a stream and bringing its
// hardware queue up at the first submission cost 15-30 ms of a 50 ms bnmf_create (a BIC sweep creates one handle per rank).
static std::mutex g_stream_mtx;
static std::vector<hipStream_t> g_stream_pool[64];
// (Round 5, measured and NOT adopted: stream priorities.  The steady iteration is 80.6 us in most processes and 83.3 us in about a quarter
// of them — in those the side-stream kernels run faster and the allocation kernel slower: how the queues' dispatches interleave differs
// from process to process (tools/ablong.py, tools/bimodal.sh).  hipStreamCreateWithPriority with the main stream high and the side streams
// low — or the reverse — makes the slow order the common one, and all three streams in one non-default class puts them on one hardware
// queue: 106-111 us.  Plain streams it is; the allocation kernel raises its waves' issue priority instead: zalloc_sort.h.)
static int take_stream(int device, hipStream_t* out, int kind = 0) {
  (void)kind;
  if (device < 0 || device >= 64) return fail(BNMF_EINVAL, "device ordinal %d out of range", device);
  {
    std::lock_guard<std::mutex> lock(g_stream_mtx);
    auto& v = g_stream_pool[device];
    if (!v.empty()) { *out = v.back(); v.pop_back(); return 0; }
  }
  HIPCHK(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
  return 0;
}
static void give_stream(int device, hipStream_t st, int kind = 0) {
  (void)kind;
  if (!st) return;
  if (device < 0 || device >= 64) { hipStreamDestroy(st); return; }
  std::lock_guard<std::mutex> lock(g_stream_mtx);
  g_stream_pool[device].push_back(st);
}
// The record_sample rings (gigabytes per handle) go back to a per-device cache at bnmf_destroy and are handed to the next handle
// that asks for the same size: releasing them and mapping new ones stalled the first kernel of the next bnmf_create by 20-30 ms (a
// BIC sweep, or bayesNMF() called in a loop, creates handle after handle of the same shape).  At most BNMF_RING_CACHE_GB (default
// 32, 0 = off) stay cached per device, oldest out first.
struct CachedBuf { void* p; size_t bytes; };
static std::mutex g_ring_mtx;
static std::vector<CachedBuf> g_ring_cache[64];
// What a destroyed handle leaves cached per device: its record_sample rings, for the next handle of the same shape (bayesNMF() after
// bayesNMF(), a BIC sweep).  Round 5: 8 GB by default (it was 32: room for one ring set of the metric configuration, 6.5 GB,
// not for several), dropped whenever a device allocation of the library fails (the allocation is then tried again), and bnmf_trim()
// releases it — and the pooled streams — on request (the library usually shares its process with PyTorch / RCCL).
static size_t ring_cache_cap() { const char* e = getenv("BNMF_RING_CACHE_GB"); return (size_t)((e ? atof(e) : 8.0) * 1e9); }
static size_t ring_cache_drop(int device) {
  std::vector<CachedBuf> drop;
  { std::lock_guard<std::mutex> lock(g_ring_mtx); if (device >= 0 && device < 64) drop.swap(g_ring_cache[device]); }
  size_t tot = 0;
  for (const auto& c : drop) { hipFree(c.p); tot += c.bytes; }
  return tot;
}
static int ring_alloc(int device, size_t bytes, double** out) {
  if (device < 0 || device >= 64) return fail(BNMF_EINVAL, "device ordinal %d out of range", device);
  {
    std::lock_guard<std::mutex> lock(g_ring_mtx);
    auto& v = g_ring_cache[device];
    for (size_t i = v.size(); i-- > 0;) if (v[i].bytes == bytes) { *out = (double*)v[i].p; v.erase(v.begin() + (long)i); return 0; }
  }
  if (hipMalloc(out, bytes) != hipSuccess) {               // out of memory with rings of other shapes cached: give them back, try once more
    (void)hipGetLastError();
    ring_cache_drop(device);
    HIPCHK(hipMalloc(out, bytes));
  }
  return 0;
}
static void ring_release(int device, void* p, size_t bytes) {
  if (!p) return;
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> lock(g_ring_mtx);
    auto& v = g_ring_cache[device];
    const size_t cap = ring_cache_cap();
    if (bytes > cap || bytes < ((size_t)1 << 20)) drop.push_back(p);        // small rings are not worth keeping
    else {
      v.push_back({p, bytes});
      size_t tot = 0;
      for (const auto& c : v) tot += c.bytes;
      while (tot > cap && !v.empty()) { tot -= v.front().bytes; drop.push_back(v.front().p); v.erase(v.begin()); }
    }
  }
  for (void* q : drop) hipFree(q);
}
// ---- who may use a device at the same time ----
// A rank-learning call takes its device exclusively, every other bnmf_run shares it (why: run_impl).  Round 5: the
// in-process gate is WRITER-PREFERRING — a std::shared_mutex of glibc admits new readers while a writer waits, so a rank-learning
// chain beside chains that keep issuing overlapping calls could wait for ever.  Here a waiting exclusive caller closes the gate for
// new sharers; those already inside finish their call (at most one block of iterations).
struct DeviceGate {
  std::mutex m; std::condition_variable cv;
  int sharers = 0, waiting_excl = 0; bool excl = false;
  unsigned long admitted_while_excl_waited = 0;           // must stay 0 (bnmf_test_gate)
  void lock_shared() {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return !excl && waiting_excl == 0; });
    if (waiting_excl) ++admitted_while_excl_waited;
    ++sharers;
  }
  void unlock_shared() { std::lock_guard<std::mutex> lk(m); if (--sharers == 0) cv.notify_all(); }
  void lock() {
    std::unique_lock<std::mutex> lk(m);
    ++waiting_excl;
    cv.wait(lk, [&] { return !excl && sharers == 0; });
    --waiting_excl; excl = true;
  }
  void unlock() { std::lock_guard<std::mutex> lk(m); excl = false; cv.notify_all(); }
};
static DeviceGate g_dev_gate[64];
// The same rule between PROCESSES: two lock files per device.  <dir>/bnmf_dev_<bus>.lock is held shared / exclusive for the length of
// a call; <dir>/bnmf_dev_<bus>.gate is the turnstile that makes it fair: an exclusive caller holds the gate exclusively from before
// it asks for the lock until it has it, a sharer passes through the gate (shared, released at once) before it asks — so sharers
// that arrive while an exclusive caller waits queue behind it (flock alone lets them overtake).
// The files: an existing one is opened read-only (flock needs no write access; O_CREAT on a file of another user in a sticky /tmp is
// refused under fs.protected_regular); a missing one is created and made world-accessible.  BNMF_LOCKDIR replaces /tmp (containers
// that share a GPU but not /tmp).  Failure is said once on stderr and remembered in the handle (run_impl refuses rank learning then).
static int open_lock_file(const char* path) {
  for (int attempt = 0; attempt < 3; ++attempt) {
    int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd >= 0) return fd;
    if (errno != ENOENT) return -1;
    fd = open(path, O_RDWR | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
    if (fd >= 0) { (void)fchmod(fd, 0666); return fd; }
    if (errno != EEXIST) return -1;                        // (EEXIST: another process has just created it — open it)
  }
  return -1;
}
static void devlock_open(const char* bus, int* lock_fd, int* gate_fd) {
  const char* dir = getenv("BNMF_LOCKDIR");
  if (!dir || !*dir) dir = "/tmp";
  char path[512];
  snprintf(path, sizeof path, "%s/bnmf_dev_%s.lock", dir, bus);
  *lock_fd = open_lock_file(path);
  const int e1 = errno;
  snprintf(path, sizeof path, "%s/bnmf_dev_%s.gate", dir, bus);
  *gate_fd = *lock_fd >= 0 ? open_lock_file(path) : -1;
  if (*lock_fd < 0 || *gate_fd < 0) {
    static std::atomic<bool> said{false};
    if (!said.exchange(true))
      fprintf(stderr, "[bnmf] warning: cannot open the device lock files %s/bnmf_dev_%s.{lock,gate} (%s): chains of OTHER processes on this device are not "
                      "kept apart from rank-learning chains; set BNMF_LOCKDIR to a directory all of them can write, or BNMF_DEVLOCK=0 if there are none\n",
              dir, bus, strerror(*lock_fd < 0 ? e1 : errno));
    if (*lock_fd >= 0) { close(*lock_fd); *lock_fd = -1; }
  }
}
// host-only checks of the two mechanisms above (tests/test_abi_host.py; no GPU involved)
extern "C" int bnmf_test_gate(int n_sharers, int calls_per_sharer, int hold_us, long* excl_wait_us, long* admitted_while_waiting) {
  // sharers keep the gate busy with overlapping calls (a reader-preferring lock would never let the exclusive caller in before they
  // stop); the exclusive caller asks once they are all running.  Reports how long it waited and how many sharers were admitted
  // while it did (must be 0).
  DeviceGate g;
  std::atomic<int> running{0};
  std::atomic<bool> stop{false};
  std::vector<std::thread> th;
  for (int i = 0; i < n_sharers; ++i)
    th.emplace_back([&, i] {
      for (int c = 0; c < calls_per_sharer && !stop.load(); ++c) {
        g.lock_shared();
        running.fetch_add(1);
        std::this_thread::sleep_for(std::chrono::microseconds(hold_us + 37 * i));
        g.unlock_shared();
      }
    });
  while (running.load() < n_sharers) std::this_thread::yield();
  const auto t0 = std::chrono::steady_clock::now();
  g.lock();
  const long waited = (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  stop.store(true);
  g.unlock();
  for (auto& t : th) t.join();
  if (excl_wait_us) *excl_wait_us = waited;
  if (admitted_while_waiting) *admitted_while_waiting = (long)g.admitted_while_excl_waited;
  return 0;
}
extern "C" int bnmf_test_devlock(const char* bus_tag, int* lock_ok, int* gate_ok) {
  int a = -1, b = -1;
  devlock_open(bus_tag ? bus_tag : "test", &a, &b);
  if (lock_ok) *lock_ok = a >= 0;
  if (gate_ok) *gate_ok = b >= 0;
  int rc = 0;
  if (a >= 0 && b >= 0) {                                  // the turnstile order of run_impl, both kinds of caller
    if (flock(b, LOCK_EX) || flock(a, LOCK_EX) || flock(b, LOCK_UN) || flock(a, LOCK_UN)) rc = -1;
    if (flock(b, LOCK_SH) || flock(b, LOCK_UN) || flock(a, LOCK_SH) || flock(a, LOCK_UN)) rc = -1;
  }
  if (a >= 0) close(a);
  if (b >= 0) close(b);
  return rc;
}
// the two static schedules as the host plans them (tests/test_schedule_host.py; no GPU involved): the call with every array NULL is the
// size query, the call with arrays fills those given.  maxM and the register kernel's N bound are derived as bnmf_create derives them.
// zsort desc: ok, KP, GBc, blocks, W, qmax, it16, pk, shared, blocks without an own column, ints of the column list as uploaded, items,
// words of Mblk, threshold blocks per cell.  zstep desc: ok, nch, workgroups, W, GBP, it16, maxfrag, batches, steps, columns, items.
extern "C" int bnmf_test_zsort_plan(int K, int G, int N, int save_Z, int n_cu, const int32_t* M, long long* desc, int32_t* blocks, int32_t* cols,
                                    uint32_t* items, uint16_t* items16, int32_t* Mblk) {
  if (!M || !desc || K < 1 || G < 1 || N < 1 || n_cu < 1) return fail(BNMF_EINVAL, "bnmf_test_zsort_plan: bad argument");
  int mx = 0;
  for (size_t i = 0; i < (size_t)K * G; ++i) { if (M[i] < 0) return fail(BNMF_EINVAL, "bnmf_test_zsort_plan: negative count in M"); if (M[i] > mx) mx = M[i]; }
  ZSortPlan p;
  if (int rc = plan_zsort(M, (size_t)K, (size_t)G, (size_t)N, save_Z != 0, mx, N <= ZNMAX, n_cu, Switches::from_env(), p)) return rc;
  const long long d[14] = {p.ok, p.KP, p.GBc, p.nb, p.W, p.qmax, p.it16, p.pk, p.shared, p.nempty, (long long)p.cols.size(), (long long)p.items.size(),
                           (long long)p.Mblk.size(), p.nblk};
  memcpy(desc, d, sizeof d);
  static_assert(sizeof(ZSBlock) == 4 * sizeof(int32_t), "ZSBlock is four ints");
  if (blocks) memcpy(blocks, p.blocks.data(), p.blocks.size() * sizeof(ZSBlock));
  if (cols) memcpy(cols, p.cols.data(), p.cols.size() * sizeof(int));
  if (items) memcpy(items, p.items.data(), p.items.size() * sizeof(uint32_t));
  if (items16) memcpy(items16, p.items16.data(), p.items16.size() * sizeof(uint16_t));
  if (Mblk) memcpy(Mblk, p.Mblk.data(), p.Mblk.size() * sizeof(int32_t));
  return 0;
}
extern "C" int bnmf_test_zstep_plan(int K, int G, int N, int save_Z, int n_cu, const int32_t* M, long long* desc, int32_t* wgs, int32_t* batches,
                                    void* steps, int32_t* cols, uint32_t* items, uint16_t* items16) {
  if (!M || !desc || K < 1 || G < 1 || N < 1 || n_cu < 1) return fail(BNMF_EINVAL, "bnmf_test_zstep_plan: bad argument");
  for (size_t i = 0; i < (size_t)K * G; ++i) if (M[i] < 0) return fail(BNMF_EINVAL, "bnmf_test_zstep_plan: negative count in M");
  ZStepPlan p;
  if (int rc = plan_zstep(M, (size_t)K, (size_t)G, (size_t)N, save_Z != 0, n_cu, Switches::from_env(), p)) return rc;
  const long long d[11] = {p.ok, p.nch, p.nwg, p.W, p.GBP, p.it16, p.maxfrag, (long long)p.batches.size(), (long long)p.steps.size(), (long long)p.cols.size(),
                           (long long)p.items.size()};
  memcpy(desc, d, sizeof d);
  static_assert(sizeof(ZPWg) == 8 && sizeof(ZPBatch) == 8 && sizeof(ZPStep) == 16, "layout of the step schedule's tables");
  if (wgs) memcpy(wgs, p.wgs.data(), p.wgs.size() * sizeof(ZPWg));
  if (batches) memcpy(batches, p.batches.data(), p.batches.size() * sizeof(ZPBatch));
  if (steps) memcpy(steps, p.steps.data(), p.steps.size() * sizeof(ZPStep));                  // { int64 item0; int32 ntw, pad; }
  if (cols) memcpy(cols, p.cols.data(), p.cols.size() * sizeof(int));
  if (items) memcpy(items, p.items.data(), p.items.size() * sizeof(uint32_t));
  if (items16) memcpy(items16, p.items16.data(), p.items16.size() * sizeof(uint16_t));
  return 0;
}

// ---- can two kernels on two streams of this device run at the same time?  (once per device and process) ----
// The steady-state sweeps hand results from the side streams to the main stream through words in memory that a lane of the
// main-stream kernel polls (kernels.h side_wait, the allocation kernels' gate): that needs the polled-for kernel to be able to
// START while the polling one is resident.  A runtime or tool that serialises dispatches (counter collection, AMD_SERIALIZE_KERNEL,
// HIP_LAUNCH_BLOCKING, a debugger, ...) breaks it — whatever its name.  The probe: kernel A on one stream spins (bounded: 2 ms)
// on a word that kernel B on another stream sets; A reports whether it saw the word.  Overlap -> flag polling; no overlap -> every
// hand-off is a stream wait on an event (serial-safe mode).  BNMF_DEBUG_PROBE=serial|overlap (tests) replaces the measurement.
__global__ void k_probe_wait(unsigned* word, unsigned* out, long long ticks_100mhz) {
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  unsigned seen = 0;
  while (!(seen = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
    if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > ticks_100mhz) break;
    __builtin_amdgcn_s_sleep(8);
  }
  *out = seen ? 1u : 2u;
}
__global__ void k_probe_set(unsigned* word) { __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static std::mutex g_probe_mtx;
static int g_probe[64];   // 0 unknown, 1 overlap, 2 serial
static int probe_overlap(int device, int* overlap) {
  std::lock_guard<std::mutex> lk(g_probe_mtx);
  if (const char* e = getenv("BNMF_DEBUG_PROBE")) {            // tests: the probe's outcome, not the mode (BNMF_SERIAL is the caller's switch)
    if (!strcmp(e, "serial")) { *overlap = 0; return 0; }
    if (!strcmp(e, "overlap")) { *overlap = 1; return 0; }
  }
  if (device < 0 || device >= 64) { *overlap = 0; return 0; }
  if (!g_probe[device]) {
    hipStream_t a = nullptr, b = nullptr;
    if (int rc = take_stream(device, &a)) return rc;
    if (int rc = take_stream(device, &b)) { give_stream(device, a); return rc; }
    unsigned* w = nullptr;
    HIPCHK(dmalloc(&w, 2 * sizeof(unsigned)));
    HIPCHK(hipMemset(w, 0, 2 * sizeof(unsigned)));
    HIPCHK(hipDeviceSynchronize());
    hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, a, w, w + 1, 200000LL);   // 2 ms of the 100 MHz counter
    hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, b, w);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(a));
    HIPCHK(hipStreamSynchronize(b));
    unsigned res[2] = {0, 0};
    HIPCHK(hipMemcpy(res, w, sizeof res, hipMemcpyDeviceToHost));
    dfree(w);
    give_stream(device, a); give_stream(device, b);
    g_probe[device] = res[1] == 1u ? 1 : 2;
    if (timing_on()) fprintf(stderr, "[bnmf] device %d: kernels on two streams %s\n", device, g_probe[device] == 1 ? "overlap" : "do NOT overlap: serial-safe mode");
  }
  *overlap = g_probe[device] == 1;
  return 0;
}
extern "C" int bnmf_trim(int device, size_t* bytes_released) {
  if (device < 0 || device >= 64) return fail(BNMF_EINVAL, "bnmf_trim: device ordinal %d out of range", device);
  HIPCHK(hipSetDevice(device));
  const size_t b = ring_cache_drop(device) + pool_drop(device);
  std::vector<hipStream_t> st;
  { std::lock_guard<std::mutex> lock(g_stream_mtx); st.swap(g_stream_pool[device]); }
  for (hipStream_t q : st) hipStreamDestroy(q);
  if (bytes_released) *bytes_released = b;
  return 0;
}
extern "C" int bnmf_probe_overlap(int device, int* overlap) {
  if (!overlap) return fail(BNMF_EINVAL, "bnmf_probe_overlap: null argument");
  HIPCHK(hipSetDevice(device));
  return probe_overlap(device, overlap);
}

static uint64_t state_data_hash(const void* p, size_t bytes);   // state_io.h

// ---- bnmf_create, step by step (create_impl at the end calls them in this order) ----
// streams, the device's lock files, events
static int create_streams(bnmf_handle* h, const Switches& sw, CreateClock& clk) {
  if (int rc = take_stream(h->device, &h->stream)) return rc;
  if (int rc = take_stream(h->device, &h->side, 1)) return rc;
  if (int rc = take_stream(h->device, &h->side2, 1)) return rc;
  clk.mark("streams");
  // one open file description per handle: flock() then also separates the handles of ONE process (BNMF_DEVLOCK=0: no file lock)
  h->devlock_off = !sw.devlock;
  if (!h->devlock_off) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus - 1, h->device) == hipSuccess) {
      for (char* c = bus; *c; ++c) if (!((*c >= '0' && *c <= '9') || (*c >= 'a' && *c <= 'z') || (*c >= 'A' && *c <= 'Z'))) *c = '_';
      devlock_open(bus, &h->devlock_fd, &h->devgate_fd);
    } else (void)hipGetLastError();
  }
  for (hipEvent_t* e : {&h->ev_draw, &h->ev_side, &h->ev_sideP, &h->ev_p, &h->ev_rank, &h->ev_z, &h->ev_red})
    HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming | hipEventDisableSystemFence));
  clk.mark("events");
  return 0;
}
// the data to the device; maxM, colmax, the data's hash.  Mf comes back pointing at the fp64 data of a Normal handle (mconv: its store
// where the caller gave counts)
static int create_data(bnmf_handle* h, const int32_t* M, const double*& Mf, std::vector<double>& mconv, CreateClock& clk) {
  const size_t KG = (size_t)h->cfg.K * h->cfg.G;
  int mx = 0;
  if (h->cfg.likelihood != BNMF_NORMAL) {
    HIPCHK(hupload(h, &h->dM, M, KG * sizeof(int32_t)));
    clk.mark("M to the device");
    for (size_t i = 0; i < KG; ++i) { if (M[i] < 0) return fail(BNMF_EINVAL, "bnmf_create: negative count in M"); if (M[i] > mx) mx = M[i]; }
    const size_t K = h->cfg.K, G = h->cfg.G;                 // (colmax is checked behind build_zsort: the sorted schedule spreads large cells over the blocks and takes more)
    for (size_t g = 0; g < G; ++g) { long cs = 0; for (size_t k = 0; k < K; ++k) cs += M[k + K * g]; if (cs > h->colmax) h->colmax = cs; }
    h->data_hash = state_data_hash(M, KG * sizeof(int32_t));
  } else {
    // a Normal handle holds its data as fp64 whichever entry point created it; nothing is sized by counts (maxM = 0: the
    // one-entry tables of create_tables, which no Normal kernel reads)
    if (M) {                                                 // Normal data given as int32 counts: converted here (exact)
      mconv.resize(KG);
      for (size_t i = 0; i < KG; ++i) { if (M[i] < 0) return fail(BNMF_EINVAL, "bnmf_create: negative count in M"); mconv[i] = (double)M[i]; }
      Mf = mconv.data();
    }
    HIPCHK(hupload(h, &h->dMf, Mf, KG * sizeof(double)));
    clk.mark("M to the device");
    h->data_hash = state_data_hash(Mf, KG * sizeof(double));
  }
  h->maxM = mx;
  return 0;
}
// the handle's own switches, the serial-safe mode, the small buffers every model needs
static int create_small(bnmf_handle* h, const Switches& sw) {
  const size_t K = h->cfg.K, G = h->cfg.G, N = h->cfg.N;
  HIPCHK(hzeroed(h, &h->dZsumK, N * G * sizeof(int32_t)));
  HIPCHK(hzeroed(h, &h->dZsumG, K * N * sizeof(int32_t)));
  if (h->cfg.save_Z) HIPCHK(hmalloc(h, &h->dZ, K * N * G * sizeof(int32_t)));
  h->gate_forced = sw.gate;
  h->mh.side_main = sw.mh_side_main; h->mh.side_tail = sw.mh_side_tail;
  h->dbg_draw_no_p = sw.draw_no_p ? 1 : 0;
  h->draw_fixed_ok = sw.draw_fixed;
  h->dbg_main_delay_us = sw.main_delay_us; h->dbg_allside_delay_us = sw.allside_delay_us; h->dbg_side_delay_us = sw.side_delay_us;
  {
    // A lane that polls inside a main-stream kernel for a side-stream kernel deadlocks (until its bound) when dispatches cannot
    // overlap: the waited-for kernel only starts once the waiting one has ended.  Where the process is known to serialise its
    // dispatches, every hand-off is a stream wait on an event instead (the structure profile mode has always used).
    // Round 5: MEASURED, not guessed from the environment (rounds 3-4 looked for AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING and the
    // profiler's variables; any other serialising tool ended in a time-out): probe_overlap runs a two-stream hand-off once per device.
    int ov = 0;
    if (int rc = probe_overlap(h->device, &ov)) return rc;
    h->serial = sw.serial >= 0 ? sw.serial != 0 : ov == 0;   // (BNMF_SERIAL: the caller's explicit choice)
  }
  HIPCHK(hzeroed(h, &h->dFlags, 64));
  HIPCHK(hmalloc(h, &h->dScal, BNMF_ID_MAX * sizeof(double)));
  HIPCHK(hzeroed(h, &h->dDrawOwn, N * sizeof(unsigned)));
  HIPCHK(hipHostMalloc((void**)&h->hErr, 64, hipHostMallocMapped));
  memset(h->hErr, 0, 64);
  HIPCHK(hipHostGetDevicePointer((void**)&h->dErr, h->hErr, 0));
  const int Rinit = (int)N;
  HIPCHK(hupload(h, &h->dR, &Rinit, sizeof(int)));
  HIPCHK(hmalloc(h, &h->dRedraw, N * sizeof(int)));
  HIPCHK(hmalloc(h, &h->dEsum, N * sizeof(double)));
  HIPCHK(hmalloc(h, &h->dPsum, N * sizeof(double)));
  HIPCHK(hmalloc(h, &h->dlpPn, 3 * N * sizeof(double)));
  h->nblkE = (int)((N * G + ES_T - 1) / ES_T);
  HIPCHK(hmalloc(h, &h->dlpE, 3 * (size_t)h->nblkE * sizeof(double)));
  HIPCHK(hmalloc(h, &h->dcol, 3 * 3 * G * sizeof(double)));   // per-column partials, 3 slots (t % 3)
  return 0;
}
// the persistent rank sweep: its exchange buffers, variant and grid (plan_rank)
static int create_rank(bnmf_handle* h, const Switches& sw) {
  const size_t K = h->cfg.K, G = h->cfg.G, N = h->cfg.N;
  const size_t gran_words = (size_t)RK_REP * 4 * 2 * ((G + RK_MAXC - 1) / RK_MAXC);   // [RK_REP copies][4 buffers][2 granules per block sum]
  HIPCHK(hzeroed(h, &h->rank.dCol, gran_words * sizeof(double)));           // tag 0 is never used
  HIPCHK(hzeroed(h, &h->rank.dSync, 32));
  const size_t rlds = (3 * N + 1) * sizeof(double);
  auto occ = [&](const void* fn) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, RK_T, rlds) != hipSuccess || nb < 1) nb = 1;
    return nb;
  };
  const bool nrm = h->cfg.likelihood == BNMF_NORMAL;
  const int occ_reg = occ(nrm ? (const void*)k_rank_sweep<true, true> : (const void*)k_rank_sweep<true, false>);
  const int occ_gen = occ(nrm ? (const void*)k_rank_sweep<false, true> : (const void*)k_rank_sweep<false, false>);
  static_cast<RankPlan&>(h->rank) = plan_rank(K, G, h->n_cu, occ_reg, occ_gen, sw);
  if (!h->rank.reg) HIPCHK(hmalloc(h, &h->rank.dMhat, K * G * sizeof(double)));
  if (sw.rank_dbg) HIPCHK(hzeroed(h, &h->rank.dDbg, (size_t)h->rank.grid * 16 * 8 * 8));   // diagnostics only
  return 0;
}
// the MH / Normal sweeps: which kernels (plan_mh), their LDS limits, their buffers, the transposed data
static int create_mh(bnmf_handle* h, const int32_t* M, const double* Mf, const Switches& sw) {
  const bnmf_config& c = h->cfg;
  const size_t K = c.K, G = c.G, N = c.N;
  Mh& m = h->mh;
  m.e_k128 = sw.mhe_k128; m.e_gw = sw.mhe_gw;
  m.no_reg = env_set("BNMF_MHREG") && !env_flag("BNMF_MHREG", true);
  if (int rc = plan_mh(K, G, N, c.MH && c.likelihood == BNMF_POISSON && !c.learning_rank, m.side_main, m.side_tail, sw, m)) return rc;
  auto raise = [](std::initializer_list<const void*> ks) {
    for (const void* kf : ks) HIPCHK(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return 0;
  };
  if (m.e_raise)
    if (int rc = raise({(const void*)k_mh_ecol<false>, (const void*)k_mh_ecol<true>, (const void*)k_mh_ecol<false, true>, (const void*)k_mh_ecol<true, true>})) return rc;
  if (m.e16_raise)
    if (int rc = raise({(const void*)k_mh_ecol16<false, false, 16>, (const void*)k_mh_ecol16<false, true, 16>, (const void*)k_mh_ecol16<false, false, 32>,
                        (const void*)k_mh_ecol16<false, true, 32>, (const void*)k_mh_ecol16<true, false, 16>, (const void*)k_mh_ecol16<true, false, 32>,
                        (const void*)k_mh_ecol16<false, false, 16, 96>, (const void*)k_mh_ecol16<false, true, 16, 96>, (const void*)k_mh_ecol16<false, false, 32, 96>,
                        (const void*)k_mh_ecol16<false, true, 32, 96>, (const void*)k_mh_ecol16<true, false, 16, 96>, (const void*)k_mh_ecol16<true, false, 32, 96>,
                        (const void*)k_mh_ecol16<false, false, 16, MHE16_KMAX, true>, (const void*)k_mh_ecol16<false, false, 32, MHE16_KMAX, true>,
                        (const void*)k_mh_ecol16<true, false, 16, MHE16_KMAX, true>, (const void*)k_mh_ecol16<true, false, 32, MHE16_KMAX, true>,
                        (const void*)k_mh_ecol16<false, false, 16, 96, true>, (const void*)k_mh_ecol16<false, false, 32, 96, true>,
                        (const void*)k_mh_ecol16<true, false, 16, 96, true>, (const void*)k_mh_ecol16<true, false, 32, 96, true>})) return rc;
  HIPCHK(hmalloc(h, &m.dMhat, 3 * K * G * sizeof(double)));      // rows of Mhat maintained by the P sweep; log(Mhat) and its candidates (MH step)
  HIPCHK(hmalloc(h, &m.dAccPn, 3 * N * sizeof(double)));
  HIPCHK(hmalloc(h, &m.dAccEpart, 3 * (size_t)h->nblkE * sizeof(double)));
  HIPCHK(hmalloc(h, &m.dNzE, 6 * N * sizeof(int)));         // nzE[N], nzP[N] (k_mh_tail's), then the hosted form's nzE[2][N], nzP[2][N] by iteration parity
  HIPCHK(hmalloc(h, &m.dEt, N * G * sizeof(double)));
  if (c.likelihood == BNMF_NORMAL) {                        // the [G][K] transpose of the data
    std::vector<double> mt(K * G);
    for (size_t g = 0; g < G; ++g) for (size_t k = 0; k < K; ++k) mt[g + G * k] = Mf[k + K * g];
    HIPCHK(hupload(h, &m.dMtf, mt.data(), K * G * sizeof(double)));
  } else {
    std::vector<int32_t> mt(K * G);
    for (size_t g = 0; g < G; ++g) for (size_t k = 0; k < K; ++k) mt[g + G * k] = M[k + K * g];
    HIPCHK(hupload(h, &m.dMt, mt.data(), K * G * sizeof(int32_t)));
  }
  return 0;
}
// the lgamma / log tables of the counts, the temperature schedule, the metric rows
static int create_tables(bnmf_handle* h, const bnmf_config* cfg, CreateClock& clk) {
  const int mx = h->maxM;
  HIPCHK(hmalloc(h, &h->dLut, 2 * (size_t)(mx + 1) * sizeof(double)));
  if (cfg->n_temperature > 0 && cfg->temperature) {
    HIPCHK(hupload(h, &h->dTemp, cfg->temperature, cfg->n_temperature * sizeof(double)));
    h->temp_host.assign(cfg->temperature, cfg->temperature + cfg->n_temperature);
  } else h->cfg.n_temperature = 0;
  h->cfg.temperature = nullptr;
  h->metrics_rows = 1024;
  HIPCHK(hipHostMalloc((void**)&h->hMetrics, h->metrics_rows * BNMF_NMETRIC * sizeof(double), hipHostMallocMapped));
  HIPCHK(hipHostGetDevicePointer((void**)&h->dMetrics, h->hMetrics, 0));
  HIPCHK(hmalloc(h, &h->dRaw, h->metrics_rows * 8 * sizeof(double)));
  hipLaunchKernelGGL(k_luts, dim3((mx + 256) / 256), dim3(256), 0, h->stream, h->dLut, h->dLut + (mx + 1), mx);
  HIPCHK(hipGetLastError());
  clk.mark("small buffers, tables");
  // wait for the tables now: left to the end of bnmf_create, the wait cost 20-25 ms on every bnmf_create after the first of a
  // process (the launch sat unsubmitted behind the allocations and copies of the schedule)
  HIPCHK(hipStreamSynchronize(h->stream));
  clk.mark("tables kernel done");
  return 0;
}
// Which allocation kernel (ZKind), its geometry or schedule.  The Poisson Gibbs sweep alone allocates counts: a Normal handle skips
// all of it (its data need not be counts).  N <= 24 takes the sorted schedule or k_zalloc_reg, larger N the step
// schedule, the tile kernel or the general LDS-search kernel k_zalloc.
static int create_zalloc(bnmf_handle* h, const int32_t* M, const Switches& sw) {
  const bnmf_config& c = h->cfg;
  const size_t K = c.K, G = c.G, N = c.N;
  if (int rc = plan_zwave(K, G, N, c.save_Z != 0, h->n_cu, sw, h->zw)) return rc;
  const bool reg_ok = h->zw.reg;
  // N > 24, stats mode: the statically scheduled lane-per-item kernel (zalloc_step.h), where its LDS layout fits
  if (!reg_ok) if (int rc = build_zstep(h, M, sw)) return rc;
  // N > 24 (or K too large for the register kernel): the tile kernel, when at least two waves per CU fit
  if (!reg_ok && h->zkind != ZKind::step) {
    static_cast<ZTilePlan&>(h->zt) = plan_ztile(K, G, N, c.save_Z != 0, h->n_cu, sw);
    if (h->zt.ok) {
      h->zkind = ZKind::tile;
      HIPCHK(hmalloc(h, &h->zt.dMhat, K * G * sizeof(double)));
      if (sw.zt_dbg) HIPCHK(hzeroed(h, &h->zt.g.dbg, 8 * sizeof(unsigned long long)));   // diagnostics only
    }
  }
  h->z_ablate = sw.ablate;
  if (h->zkind == ZKind::none && !h->z_ablate) if (int rc = build_zsort(h, M, reg_ok, sw)) return rc;
  if (h->zkind == ZKind::none) h->zkind = reg_ok ? ZKind::reg : ZKind::general;
  // the other allocation kernels take a column whole (k_zalloc_reg: one wave per column; tile / step: a workgroup's batch): 4,000,000 counts
  // per column is where that stops being a sensible launch.  The sorted schedule (N <= 24, K <= 1,024, no save_Z) spreads the counts of a
  // large cell over all blocks and is bounded by its item format only (a cell <= 65,534 fragments of 256 counts = 16.7 M counts).
  if (h->colmax > 4000000 && !(h->zkind == ZKind::sort && h->zs.shared))
    return fail(BNMF_EINVAL, "bnmf_create: a column of M sums to %ld (> 4,000,000 counts): unsupported for this model / shape (N <= 24 and K <= 1,024 without save_Z take up to 16.7 M counts per cell)", h->colmax);
  return 0;
}

static int create_impl(const bnmf_config* cfg, const int32_t* M, const double* Mf, bnmf_handle* h) {
  const bool normal = cfg->likelihood == BNMF_NORMAL;
  const Switches sw = Switches::from_env();
  CreateClock clk;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
  h->n_cu = prop.multiProcessorCount;
  std::vector<double> mconv;
  if (int rc = create_streams(h, sw, clk)) return rc;
  if (int rc = create_data(h, M, Mf, mconv, clk)) return rc;
  if (int rc = create_small(h, sw)) return rc;
  if (cfg->learning_rank) if (int rc = create_rank(h, sw)) return rc;
  if (cfg->MH || normal) if (int rc = create_mh(h, M, Mf, sw)) return rc;
  if (int rc = create_tables(h, cfg, clk)) return rc;
  if (!normal) if (int rc = create_zalloc(h, M, sw)) return rc;
  clk.mark("allocation-kernel schedule");
  HIPCHK(hipStreamSynchronize(h->stream));
  refresh_dev(h);
  clk.mark("drain");
  return 0;
}

int bnmf_destroy(bnmf_handle* h) {
  if (!h) return 0;
  hipSetDevice(h->device);
  for (hipStream_t st : {h->stream, h->side, h->side2}) if (st) hipStreamSynchronize(st);
  for (int id = 0; id < BNMF_ID_MAX; ++id) {
    Arr& a = h->arr[id];
    if (!a.slab) dfree(a.d);
    ring_release(h->device, a.ring, (size_t)h->wcap * id_len(h, id) * sizeof(double));
  }
  dfree(h->E_alt);                                         // (trades places with Arr::d of E every sweep: released like one, not owned)
  for (void* p : h->owned) dfree(p);                       // every other pooled device block, in the order made
  for (void* p : {(void*)h->hMetrics, (void*)h->hErr, (void*)h->hStage}) if (p) hipHostFree(p);
  for (hipEvent_t e : {h->ev_draw, h->ev_side, h->ev_sideP, h->ev_p, h->ev_rank, h->ev_z, h->ev_red}) if (e) hipEventDestroy(e);
  if (h->have_ev) for (auto& e : h->ev) hipEventDestroy(e);
  if (h->devlock_fd >= 0) close(h->devlock_fd);
  if (h->devgate_fd >= 0) close(h->devgate_fd);
  give_stream(h->device, h->side, 1); give_stream(h->device, h->side2, 1);
  give_stream(h->device, h->stream);                    // synchronised at the top of this function
  delete h;
  return 0;
}

int bnmf_set_array(bnmf_handle* h, int id, const double* x, size_t n) {
  if (!h || !x) return fail(BNMF_EINVAL, "bnmf_set_array: null argument");
  const size_t len = id_len(h, id);
  if (len == 0) return fail(BNMF_EINVAL, "bnmf_set_array: unknown id %d", id);
  HIPCHK(hipSetDevice(h->device));
  CreateClock clk;
  HIPCHK(hipStreamSynchronize(h->stream));
  clk.mark("set_array: sync main");
  HIPCHK(hipStreamSynchronize(h->side));
  clk.mark("set_array: sync side");
  HIPCHK(hipStreamSynchronize(h->side2));
  clk.mark("set_array: sync side2");
  h->pipe.invalidate_prepared();   // state changed: the pre-issued k_side must be redone
  if (id == BNMF_R) { int r = (int)x[0]; HIPCHK(hipMemcpy(h->dR, &r, sizeof(int), hipMemcpyHostToDevice)); h->arr[BNMF_R].set = true; return 0; }
  if (id == BNMF_ZSUMK || id == BNMF_ZSUMG || id == BNMF_Z) {
    int32_t* dst = id == BNMF_ZSUMK ? h->dZsumK : id == BNMF_ZSUMG ? h->dZsumG : h->dZ;
    if (!dst) return fail(BNMF_EUNSET, "bnmf_set_array: Z is not materialised (save_Z = 0)");
    if (n != len) return fail(BNMF_ESIZE, "bnmf_set_array: id %d expects %zu values, got %zu", id, len, n);
    std::vector<int32_t> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = (int32_t)x[i];
    HIPCHK(hipMemcpy(dst, tmp.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    if (id == BNMF_Z) h->pipe.z_expanded_iter = h->iter;        // (what the caller stored is what a read returns until the next sweep)
    return 0;
  }
  Arr& a = h->arr[id];
  if (is_hyper(id) && n == 1) {
    // a broadcast scalar lives in the handle's block of scalars: the eight device allocations of the default hyper-prior values
    // were 20 ms of a bayesNMF() call
    if (a.d && !a.slab) HIPCHK(dfree(a.d));
    a.d = h->dScal + id; a.slab = true;
    // the value travels as a kernel argument: the first small host-to-device copy of a handle created after another one had been
    // destroyed took 13-24 ms (BNMF_TIMING marks), every time
    hipLaunchKernelGGL(k_set_scalar, dim3(1), dim3(1), 0, h->stream, a.d, x[0]);
    HIPCHK(hipGetLastError());
    clk.mark("set_array: a scalar");
    a.n = 1; a.stride = 0; a.set = true;
    refresh_dev(h);
    return 0;
  }
  if (n != len) return fail(BNMF_ESIZE, "bnmf_set_array: id %d expects %zu values, got %zu", id, len, n);
  const size_t nslot = is_prior_param(id) ? 2 : 1;
  if (a.d && (a.n != len || a.slab)) { if (!a.slab) HIPCHK(dfree(a.d)); a.d = nullptr; a.slab = false; }
  if (!a.d) HIPCHK(dmalloc(&a.d, nslot * len * sizeof(double)));
  HIPCHK(hipMemcpy(a.d + (nslot == 2 ? (size_t)cur_slot(h) * len : 0), x, len * sizeof(double), hipMemcpyHostToDevice));
  a.n = len; a.stride = 1; a.set = true;
  // which columns n (P side) / rows n (E side) carry a missing (NaN) entry
  if (!is_hyper(id) && len >= (size_t)h->cfg.N && id != BNMF_A && id < 30) {
    const size_t K = h->cfg.K, N = h->cfg.N;
    a.redraw.assign(N, 0);
    const bool ps = is_pside(id);
    for (size_t i = 0; i < len; ++i) if (x[i] != x[i]) a.redraw[ps ? i / K : i % N] = 1;
  }
  refresh_dev(h);
  return 0;
}

int bnmf_get_array(bnmf_handle* h, int id, double* out, size_t n) {
  if (!h || !out) return fail(BNMF_EINVAL, "bnmf_get_array: null argument");
  if (h->poisoned) return fail(BNMF_ESTATE, "bnmf_get_array: the handle timed out inside a kernel; its state is invalid");
  const size_t len = id_len(h, id);
  if (len == 0 || n != len) return fail(BNMF_ESIZE, "bnmf_get_array: id %d expects %zu values, got %zu", id, len, n);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->side));
  HIPCHK(hipStreamSynchronize(h->side2));
  if (id == BNMF_R) { int r; HIPCHK(hipMemcpy(&r, h->dR, sizeof(int), hipMemcpyDeviceToHost)); out[0] = r; return 0; }
  if (id == BNMF_ZSUMK || id == BNMF_ZSUMG || id == BNMF_Z) {
    const int32_t* src = id == BNMF_ZSUMK ? h->dZsumK : id == BNMF_ZSUMG ? h->dZsumG : h->dZ;
    if (!src) return fail(BNMF_EUNSET, "bnmf_get_array: Z is not materialised (save_Z = 0)");
    if (id == BNMF_Z) if (int rc = ensure_Z(h)) return rc;
    std::vector<int32_t> tmp(n);
    HIPCHK(hipMemcpy(tmp.data(), src, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = tmp[i];
    return 0;
  }
  if (id == BNMF_MHAT) {
    // the rows of Mhat as the last row sweep of the MH / Normal models left them: P_t diag(A) E_{t-1}, maintained factor by factor
    if (!h->mh.dMhat || h->iter < 2) return fail(BNMF_EUNSET, "bnmf_get_array: Mhat is maintained by the row sweep of the MH / Normal models, after their first iteration");
    if (h->mh.S <= MHP_W && !h->mh.no_reg)
      return fail(BNMF_EUNSET, "bnmf_get_array: this handle's row sweep keeps Mhat in registers; create it with BNMF_MHREG=0 to read it");
    const size_t K = h->cfg.K, G = h->cfg.G;
    std::vector<double> rows(K * G);
    HIPCHK(hipMemcpy(rows.data(), h->mh.dMhat, K * G * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < K; ++k) for (size_t g = 0; g < G; ++g) out[k + K * g] = rows[k * G + g];
    return 0;
  }
  const Arr& a = h->arr[id];
  if (!a.d) return fail(BNMF_EUNSET, "bnmf_get_array: id %d has no value", id);
  if (a.stride == 0) { double v; HIPCHK(hipMemcpy(&v, a.d, sizeof(double), hipMemcpyDeviceToHost)); for (size_t i = 0; i < n; ++i) out[i] = v; return 0; }
  HIPCHK(hipMemcpy(out, a.d + (is_prior_param(id) ? (size_t)cur_slot(h) * len : 0), n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int bnmf_get_array_i32(bnmf_handle* h, int id, int32_t* out, size_t n) {
  if (!h || !out) return fail(BNMF_EINVAL, "bnmf_get_array_i32: null argument");
  const size_t len = id_len(h, id);
  const int32_t* src = id == BNMF_ZSUMK ? h->dZsumK : id == BNMF_ZSUMG ? h->dZsumG : id == BNMF_Z ? h->dZ : nullptr;
  if (!(id == BNMF_ZSUMK || id == BNMF_ZSUMG || id == BNMF_Z)) return fail(BNMF_EINVAL, "bnmf_get_array_i32: id %d is not an integer array", id);
  if (!src) return fail(BNMF_EUNSET, "bnmf_get_array_i32: Z is not materialised (save_Z = 0)");
  if (n != len) return fail(BNMF_ESIZE, "bnmf_get_array_i32: id %d expects %zu values, got %zu", id, len, n);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (id == BNMF_Z) if (int rc = ensure_Z(h)) return rc;
  HIPCHK(hipMemcpy(out, src, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}

int bnmf_debug_rank(bnmf_handle* h, unsigned long long* out, size_t n) {   // diagnostics: phase time stamps of k_rank_sweep
  if (!h || !h->rank.dDbg) return fail(BNMF_ESTATE, "BNMF_RANKDBG not set");
  HIPCHK(hipMemcpy(out, h->rank.dDbg, n * 8, hipMemcpyDeviceToHost));
  return h->rank.grid;
}
#ifdef ZSPROF
int bnmf_debug_zstamps(bnmf_handle* h, unsigned long long* out) {   // diagnostics (-DZSPROF): [3 blocks][16 waves][8] s_memrealtime stamps of the last k_zalloc_sort
  if (!h || !h->zs.dProf) return fail(BNMF_ESTATE, "not a -DZSPROF build, or the kernel is not in use");
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(out, h->zs.dProf + 8, 3 * 16 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}
#endif
int bnmf_debug_zsort(bnmf_handle* h, unsigned long long* out) {   // diagnostics (-DZSPROF / -DZPPROF builds): section ticks of k_zalloc_sort / k_zalloc_step, then reset
  unsigned long long* src = h ? (h->zs.dProf ? h->zs.dProf : h->zp.g.prof) : nullptr;
  if (!src) return fail(BNMF_ESTATE, "not a -DZSPROF / -DZPPROF build, or the kernel is not in use");
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(out, src, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(src, 0, 8 * sizeof(unsigned long long)));
  return 0;
}
#ifdef ZSPROF
int bnmf_debug_draw(bnmf_handle* h, unsigned long long* out, int reset) {   // diagnostics (-DZSPROF builds): [wave][8] section ticks of k_draw's E waves
  if (!h) return fail(BNMF_EINVAL, "null");
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_drprof), 8 * DRPROF_W * sizeof(unsigned long long)));
  if (reset) {
    std::vector<unsigned long long> z(8 * DRPROF_W, 0ull);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_drprof), z.data(), z.size() * sizeof(unsigned long long)));
  }
  return DRPROF_W;
}
#endif
int bnmf_debug_set_timeout(bnmf_handle* h, int word) {   // tests: what a bounded in-kernel wait does when it gives up
  if (!h || word < 0 || word > 1) return fail(BNMF_EINVAL, "bnmf_debug_set_timeout: bad argument");
  ((volatile int*)h->hErr)[word] = 2;
  return 0;
}
int bnmf_get_stat(bnmf_handle* h, int what, double* out) {   // sizes of the schedule's buffers, for bench.py's byte counts
  if (!h || !out) return fail(BNMF_EINVAL, "bnmf_get_stat: null argument");
  switch (what) {
    case 0: *out = (double)h->zs.recwords * 4.0; return 0;                                  // bytes of item records per iteration (save_Z, sorted schedule; else 0)
    case 1: *out = h->zs.dMh ? (double)h->cfg.K * h->cfg.G * 8.0 : 0.0; return 0;            // bytes of Mhat left per iteration for the column terms
    case 2: *out = h->zs.dRecRing ? 1.0 : 0.0; return 0;                                     // samples$Z kept as a ring of records
    case 3: *out = h->zs.eager ? 1.0 : 0.0; return 0;
    case 5: *out = h->zkind == ZKind::sort ? (double)h->zs.qmax : 0.0; return 0;                          // quads per item of the sorted schedule (chosen per data set)
    case 4: *out = h->mh.pipe ? 1.0 : 0.0; return 0;                                        // MH sweep: k_mh_tail's work hosted by the two sweep kernels
    case 6: *out = h->zkind == ZKind::sort ? (double)h->zs.g.nblocks : h->zkind == ZKind::step ? (double)h->zp.g.nwg : 0.0; return 0;   // blocks (workgroups) of the static schedule
    case 7: *out = h->zkind == ZKind::sort ? (double)h->zs.nempty : 0.0; return 0;                        // ... of them without an own column (k_zalloc_step: never)
    case 8: *out = (double)h->n_fixed; return 0;                                            // columns of P held fixed (bnmf_set_fixed)
    case 9: *out = !h->mh.dMhat ? 0.0 : (h->mh.S <= MHP_W && !h->mh.no_reg) ? 1.0 : 2.0; return 0;   // MH / Normal row sweep: 1 its register form, 2 the form with Mhat in memory
    case 10: *out = (double)h->draw_seq; return 0;                                          // launches of the merged draw kernel so far
    case 11: *out = h->zkind == ZKind::step ? 1.0 : 0.0; return 0;                          // the allocation kernel is k_zalloc_step
    default: return fail(BNMF_EINVAL, "bnmf_get_stat: unknown statistic %d", what);
  }
}
int bnmf_get_iter(bnmf_handle* h, int* iter) { if (!h || !iter) return fail(BNMF_EINVAL, "null"); *iter = h->iter; return 0; }

// the mask of fixed columns on the handle and on the device (bnmf_set_fixed, bnmf_load_state); a mask of zeros leaves Dev::fixedP null:
// the kernels then run the path they run without a mask
static int apply_fixed(bnmf_handle* h, const int32_t* fixed) {
  const size_t N = h->cfg.N;
  HIPCHK(hipSetDevice(h->device));
  if (!h->dFixedP) HIPCHK(hmalloc(h, &h->dFixedP, N * sizeof(int)));
  HIPCHK(hipMemcpy(h->dFixedP, fixed, N * sizeof(int), hipMemcpyHostToDevice));
  h->fixedP.assign(fixed, fixed + N);
  h->n_fixed = 0;
  for (size_t n = 0; n < N; ++n) h->n_fixed += fixed[n] != 0;
  refresh_dev(h);
  return 0;
}
int bnmf_set_fixed(bnmf_handle* h, int id, const int32_t* fixed, size_t n) {
  if (!h || !fixed) return fail(BNMF_EINVAL, "bnmf_set_fixed: null argument");
  if (id != BNMF_P) return fail(BNMF_EMODEL, "bnmf_set_fixed: only columns of P (id %d) can be held fixed, not id %d (fixing rows of E is out of scope)", (int)BNMF_P, id);
  if (n != (size_t)h->cfg.N) return fail(BNMF_ESIZE, "bnmf_set_fixed: the mask has %zu entries, P has N = %d columns", n, h->cfg.N);
  for (size_t i = 0; i < n; ++i)
    if (fixed[i] != 0 && fixed[i] != 1) return fail(BNMF_EINVAL, "bnmf_set_fixed: fixed[%zu] = %d (column %zu) is neither 0 nor 1", i, (int)fixed[i], i);
  if (h->inited || h->iter != 0)
    return fail(BNMF_ESTATE, "bnmf_set_fixed: the handle has been initialised, loaded or run (iteration %d); set the mask before bnmf_init / bnmf_load_state", h->iter);
  return apply_fixed(h, fixed);
}
int bnmf_get_fixed(bnmf_handle* h, int id, int32_t* out, size_t n) {
  if (!h || !out) return fail(BNMF_EINVAL, "bnmf_get_fixed: null argument");
  if (id != BNMF_P) return fail(BNMF_EMODEL, "bnmf_get_fixed: only columns of P (id %d) can be held fixed, not id %d", (int)BNMF_P, id);
  if (n != (size_t)h->cfg.N) return fail(BNMF_ESIZE, "bnmf_get_fixed: the mask has N = %d entries, room for %zu given", h->cfg.N, n);
  for (size_t i = 0; i < n; ++i) out[i] = h->fixedP.empty() ? 0 : h->fixedP[i];
  return 0;
}
// bnmf_init with fixed columns: each must hold a usable value — decided on the host (P is read back, nothing is written)
static int check_fixed_columns(bnmf_handle* h) {
  if (h->n_fixed == 0) return 0;
  const size_t K = h->cfg.K, N = h->cfg.N;
  const Arr& a = h->arr[BNMF_P];
  size_t first = 0;
  while (!h->fixedP[first]) ++first;
  if (!a.set || !a.d) return fail(BNMF_EUNSET, "bnmf_init: column %zu of P is fixed but P has no value (bnmf_set_array(BNMF_P) first)", first);
  std::vector<double> P(K * N);
  HIPCHK(hipMemcpy(P.data(), a.d, K * N * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t n = 0; n < N; ++n) {
    if (!h->fixedP[n]) continue;
    double sum = 0.0;
    for (size_t k = 0; k < K; ++k) {
      const double v = P[k + K * n];
      if (v != v) return fail(BNMF_EUNSET, "bnmf_init: fixed column %zu of P has no value at row %zu (NaN)", n, k);
      if (v < 0.0 || std::isinf(v)) return fail(BNMF_EINVAL, "bnmf_init: fixed column %zu of P holds %g at row %zu (a signature is finite and non-negative)", n, v, k);
      sum += v;
    }
    if (sum == 0.0) return fail(BNMF_EINVAL, "bnmf_init: fixed column %zu of P sums to 0", n);
  }
  return 0;
}

}  // extern "C"

#include "sweep.h"   // the scheduler: launch helpers, sweep / sweep_mh / sweep_mh_pipe, run_impl

extern "C" {

int bnmf_init(bnmf_handle* h, double* metrics_row1) {
  if (!h) return fail(BNMF_EINVAL, "bnmf_init: null handle");
  HIPCHK(hipSetDevice(h->device));
  if (h->poisoned) return fail(BNMF_ESTATE, "bnmf_init: the handle timed out inside a kernel; destroy it");
  if (int rc = check_fixed_columns(h)) return rc;
  if (h->inited) {
    // Re-initialisation restarts the iteration counter at 1, and with it every epoch the kernels compare their sync words
    // against (flags < epoch, the rank sweep's granule tags): stale words from the first life of the handle would satisfy
    // those waits at once.  Drain the streams and clear the words and the host-side pipeline state.
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));
    HIPCHK(hipStreamSynchronize(h->side2));
    HIPCHK(hipMemset(h->dFlags, 0, 64));
    memset(h->hErr, 0, 64);
    if (h->rank.dSync) HIPCHK(hipMemset(h->rank.dSync, 0, 32));
    if (h->rank.dCol) HIPCHK(hipMemset(h->rank.dCol, 0, (size_t)RK_REP * 4 * 2 * (((size_t)h->cfg.G + RK_MAXC - 1) / RK_MAXC) * sizeof(double)));
    HIPCHK(hipMemset(h->dZsumK, 0, (size_t)h->cfg.N * h->cfg.G * sizeof(int32_t)));
    HIPCHK(hipMemset(h->dZsumG, 0, (size_t)h->cfg.K * h->cfg.N * sizeof(int32_t)));
    h->pipe = Pipe{};
    h->inited = false;
  }
  const bnmf_config& c = h->cfg;
  const int N = c.N;
  const long KN = (long)c.K * N, NG = (long)N * c.G;
  // the prior parameters of iteration 1, drawn from their hyper-priors: gamma variates (k_init_gamma, from the hyper-prior pair hs, hr)
  // or, for the truncated-normal prior, Mu / Sigmasq (k_init_tn)
  struct Spec { int id; uint32_t var; int side; int hs, hr, is_mu; };   // hs < 0: k_init_tn
  std::vector<Spec> specs;
  if (c.prior == BNMF_GAMMA) {
    if (int rc = need_hyper(h, {BNMF_HA_P, BNMF_HB_P, BNMF_HC_P, BNMF_HD_P, BNMF_HA_E, BNMF_HB_E, BNMF_HC_E, BNMF_HD_E})) return rc;
    specs = {{BNMF_BETA_P, BNMF_V_BETA_P, 0, BNMF_HA_P, BNMF_HB_P, 0}, {BNMF_ALPHA_P, BNMF_V_ALPHA_P, 0, BNMF_HC_P, BNMF_HD_P, 0},
             {BNMF_BETA_E, BNMF_V_BETA_E, 1, BNMF_HA_E, BNMF_HB_E, 0}, {BNMF_ALPHA_E, BNMF_V_ALPHA_E, 1, BNMF_HC_E, BNMF_HD_E, 0}};
  } else if (c.prior == BNMF_EXPONENTIAL) {
    if (int rc = need_hyper(h, {BNMF_HA_P, BNMF_HB_P, BNMF_HA_E, BNMF_HB_E})) return rc;
    specs = {{BNMF_LAMBDA_P, BNMF_V_LAMBDA_P, 0, BNMF_HA_P, BNMF_HB_P, 0}, {BNMF_LAMBDA_E, BNMF_V_LAMBDA_E, 1, BNMF_HA_E, BNMF_HB_E, 0}};
  } else if (c.prior == BNMF_TRUNCNORMAL) {
    if (int rc = need_hyper(h, {BNMF_HM_P, BNMF_HS_P, BNMF_HA_P, BNMF_HB_P, BNMF_HM_E, BNMF_HS_E, BNMF_HA_E, BNMF_HB_E})) return rc;
    specs = {{BNMF_MU_P, BNMF_V_MU_P, 0, -1, -1, 1}, {BNMF_SIGMASQ_P, BNMF_V_SIGSQ_P, 0, -1, -1, 0}, {BNMF_MU_E, BNMF_V_MU_E, 1, -1, -1, 1}, {BNMF_SIGMASQ_E, BNMF_V_SIGSQ_E, 1, -1, -1, 0}};
  }
  for (const Spec& sp : specs) {
    Arr& a = h->arr[sp.id];
    std::vector<int> redraw(N, 1);
    if (a.set) redraw = a.redraw.empty() ? std::vector<int>(N, 0) : a.redraw;
    if (int rc = ensure(h, sp.id)) return rc;
    refresh_dev(h);
    HIPCHK(hipMemcpyAsync(h->dRedraw, redraw.data(), N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    const long len = sp.side ? NG : KN;
    double* slot1 = a.d + (size_t)len;                      // iteration 1 lives in slot 1
    auto go = [&](auto kernP, auto kernE, auto... args) {
      auto kern = sp.side ? kernE : kernP;
      hipLaunchKernelGGL(kern, dim3((len + 255) / 256), dim3(256), 0, h->stream, h->dev, slot1, args..., sp.var, h->dRedraw);
    };
    if (sp.hs >= 0) go(k_init_gamma<0>, k_init_gamma<1>, HRef{h->arr[sp.hs].d, h->arr[sp.hs].stride}, HRef{h->arr[sp.hr].d, h->arr[sp.hr].stride});
    else go(k_init_tn<0>, k_init_tn<1>, sp.is_mu);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));   // redraw is reused by the next spec
  }
  const bool haveP = h->arr[BNMF_P].set, haveE = h->arr[BNMF_E].set, haveA = h->arr[BNMF_A].set;
  if (int rc = ensure(h, BNMF_P)) return rc;
  if (int rc = ensure(h, BNMF_E)) return rc;
  if (int rc = ensure(h, BNMF_A)) return rc;
  if (c.MH) { if (int rc = ensure(h, BNMF_ACC_P)) return rc; if (int rc = ensure(h, BNMF_ACC_E)) return rc; }
  if (c.likelihood == BNMF_NORMAL) {
    const double three = 3.0;                                   // alpha = beta = 3 (R/bayesNMF_sampler.R:222-230)
    if (!h->arr[BNMF_ALPHA].d) if (int rc = bnmf_set_array(h, BNMF_ALPHA, &three, 1)) return rc;
    if (!h->arr[BNMF_BETA].d) if (int rc = bnmf_set_array(h, BNMF_BETA, &three, 1)) return rc;
    if (int rc = ensure(h, BNMF_SIGMASQ)) return rc;
  }
  if (!haveA) { std::vector<double> ones(N, 1.0); HIPCHK(hipMemcpy(h->arr[BNMF_A].d, ones.data(), N * sizeof(double), hipMemcpyHostToDevice)); }
  refresh_dev(h);
  h->iter = 1;
  Timer tm{h, false};
  use_slot(h, 1u);
  if (int rc = ensure_rings(h)) return rc;
  // skip = names(init_params): supplied P / E kept verbatim.  With fixed columns the OTHER columns of a supplied P that carry a missing
  // (NaN) entry are drawn from the prior, as missing columns of the prior parameters are: the launch keeps the columns of a mask of its own
  std::vector<int> keepP;
  if (haveP && h->n_fixed > 0 && !h->arr[BNMF_P].redraw.empty())
    for (int n = 0; n < N; ++n) if (h->arr[BNMF_P].redraw[n] && !h->fixedP[n]) { keepP.assign(N, 1); break; }
  if (!keepP.empty()) {
    for (int n = 0; n < N; ++n) keepP[n] = (h->arr[BNMF_P].redraw[n] && !h->fixedP[n]) ? 0 : 1;
    HIPCHK(hipMemcpy(h->dRedraw, keepP.data(), N * sizeof(int), hipMemcpyHostToDevice));
    launch_pdraw(h, 1u, 1, false, h->dRedraw);
  } else {
    launch_pdraw(h, 1u, haveP ? 2 : 1, false);
  }
  launch_edraw(h, 1u, haveE ? 2 : 1, false);                // (iteration 1 is recorded by k_record below, every model)
  launch_side(h, 2u, tm);
  if (!haveA && c.learning_rank) {                            // R ~ Uniform{0..N}, A[n] ~ Bernoulli(pi(R))
    hipLaunchKernelGGL(k_rank_R, dim3(1), dim3(64), (size_t)(N + 1) * sizeof(double), h->stream, h->dev, 1u, 1);
    hipLaunchKernelGGL(k_rank_Aprior, dim3((N + 63) / 64), dim3(64), 0, h->stream, h->dev, 1u);
  }
  if (c.MH || c.likelihood == BNMF_NORMAL) launch_mh_metrics(h, 1u, true);
  else { if (int rc = launch_zalloc(h, 1u)) return rc; if (h->zkind == ZKind::sort) { h->pipe.ct_pending = 1u; flush_colterms(h); } record_Z(h, 1u); }
  if (int rc = launch_record(h, 1u)) return rc;
  launch_reduce(h, 1u, 0, tm);
  flush_reduce(h, tm);
  hipEventRecord(h->ev_z, h->side); hipStreamWaitEvent(h->stream, h->ev_z, 0);
  hipLaunchKernelGGL(k_compose, dim3(1), dim3(64), 0, h->stream, h->dev, 1, 1u);
  HIPCHK(hipGetLastError());
  double row1[BNMF_NMETRIC];
  HIPCHK(hipStreamSynchronize(h->stream));
  memcpy(row1, h->hMetrics, BNMF_NMETRIC * sizeof(double));
  HIPCHK(hipStreamSynchronize(h->side));
  HIPCHK(hipStreamSynchronize(h->side2));
  if (metrics_row1) memcpy(metrics_row1, row1, sizeof row1);
  if (h->wcap > 0) { h->hist.assign((size_t)h->wcap * 4, std::nan("")); h->hist[0] = row1[3]; h->hist[1] = row1[4]; h->hist[2] = row1[9]; h->hist[3] = row1[10]; }
  h->inited = true;
  return 0;
}

int bnmf_run(bnmf_handle* h, int n_iter, int converged, double* metrics) {
  Timer tm{h, false};
  return run_impl(h, n_iter, converged, metrics, tm);
}
int bnmf_profile(bnmf_handle* h, int n_iter, int converged, double* out_ms) {
  if (!h || !out_ms) return fail(BNMF_EINVAL, "bnmf_profile: null argument");
  HIPCHK(hipSetDevice(h->device));
  if (!h->have_ev) { for (auto& e : h->ev) HIPCHK(hipEventCreate(&e)); h->have_ev = true; }
  Timer tm{h, true};
  if (int rc = run_impl(h, n_iter, converged, nullptr, tm)) return rc;
  for (int k = 0; k < BNMF_NKERNEL; ++k) out_ms[k] = tm.cnt[k] ? tm.acc[k] / tm.cnt[k] : 0.0;
  return 0;
}
}  // extern "C"

#include "posterior.h"   // the posterior calls on a recorded range and the layer they share

extern "C" {

int bnmf_window(bnmf_handle* h, int id, int last_n, double* out) {
  if (!h || !out) return fail(BNMF_EINVAL, "bnmf_window: null argument");
  if (int rc = check_recorded(h, "bnmf_window")) return rc;
  if (int rc = check_last(h, "bnmf_window", last_n)) return rc;
  if (id < 0 || id >= BNMF_ID_MAX) return fail(BNMF_EINVAL, "bnmf_window: unknown id %d", id);
  if (id == BNMF_Z) {
    if (!h->zring && !h->zs.dRecRing) return fail(BNMF_EUNSET, "bnmf_window: Z is not kept per sample (needs save_Z, a window, and the window's samples within BNMF_ZRING_GB)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t lenz = id_len(h, BNMF_Z);
    std::vector<int32_t> tmp(lenz);
    for (int i = 0; i < last_n; ++i) {
      const size_t slot = (size_t)(h->iter - last_n + i) % (size_t)h->wcap;
      if (h->zs.dRecRing) {                                   // sorted schedule: the sample is its item records; expand them (k_zexpand) and copy
        launch_zexpand(h, (uint32_t)(h->iter - last_n + i + 1));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(tmp.data(), h->dZ, lenz * sizeof(int32_t), hipMemcpyDeviceToHost));
      } else
      HIPCHK(hipMemcpy(tmp.data(), h->zring + slot * lenz, lenz * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (size_t j = 0; j < lenz; ++j) out[(size_t)i * lenz + j] = tmp[j];
    }
    return 0;
  }
  if (!h->arr[id].ring || id_len(h, id) == 0) return fail(BNMF_EUNSET, "bnmf_window: id %d is not recorded for this model", id);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return ring_read(h, id, h->iter, last_n, out);
}


// One MAP check (R/bayesNMF_sampler.R:297-321): get_MAP_ over the last min(MAP_over, iter) samples on the device, the
// state$MAP_metrics row (update_MAP_metrics_, R/utils.R:356-397) and check_convergence_ (R/convergence.R:60-154) into mr.
static int map_check(bnmf_handle* h, const bnmf_convergence_control* cc, bnmf_convergence_state* st, const double* lastrow, double* mr,
                     std::vector<double>& Am, std::vector<int32_t>& used) {
  const int K = h->cfg.K, G = h->cfg.G, N = h->cfg.N;
  const int it = h->iter;
  const int win = it < cc->MAP_over ? it : cc->MAP_over;
  bnmf_map_info info;
  if (int rc = bnmf_map(h, win, 0.0, nullptr, nullptr, Am.data(), nullptr, nullptr, nullptr, nullptr, nullptr, used.data(), &info)) return rc;
  // update_MAP_metrics_: loglikelihood / logposterior are means of the per-sample values over the whole window
  double ll = 0.0, lp = 0.0, mt = 0.0, sumA = 0.0;
  for (int i = it - win + 1; i <= it; ++i) {
    const double* hrow = h->hist.data() + (size_t)((i - 1) % h->wcap) * 4;
    ll += hrow[0]; lp += hrow[1];
    mt += h->temp_host.empty() ? 1.0 : h->temp_host[std::min<size_t>((size_t)i - 1, h->temp_host.size() - 1)];
  }
  ll /= win; lp /= win; mt /= win;
  for (int j = 0; j < N; ++j) sumA += Am[j];
  const double n_params = sumA * (double)(G + K);
  mr[0] = it; mr[1] = info.rmse; mr[2] = info.kl; mr[3] = ll; mr[4] = lp; mr[5] = n_params;
  mr[6] = -2.0 * ll + n_params * std::log((double)G); mr[7] = sumA; mr[8] = info.top_counts[0]; mr[9] = mt;
  mr[10] = lastrow[9]; mr[11] = lastrow[10];            // compute_metrics_ uses the CURRENT acceptance matrices
  // check_convergence_
  static const int col_of[5] = {3, 4, 1, 2, 6};
  double m = mr[col_of[cc->metric]];
  if (cc->metric <= 1) m = -m;
  if (!st->have_prev) { st->prev_MAP_metric = m + 1.0; st->best_MAP_metric = m + 1.0; st->inarow_na = st->inarow_no_change = st->inarow_no_best = 0; st->have_prev = 1; }
  const double pc = (m - st->prev_MAP_metric) / st->prev_MAP_metric;
  st->prev_percent_change = pc; st->prev_MAP_metric = m;
  if (pc != pc) { st->inarow_no_change = 0; st->inarow_no_best = 0; st->inarow_na += 1; }
  else if (std::fabs(pc) < cc->tol) { st->inarow_no_change += 1; st->inarow_na = 0; }
  else { st->inarow_no_change = 0; st->inarow_na = 0; }
  bool temps_one = true;                                  // temperature_schedule[(iter - MAP_over):iter] == 1 (R drops index 0)
  for (int i = std::max(it - cc->MAP_over, 1); i <= it && temps_one; ++i)
    temps_one = h->temp_host.empty() || h->temp_host[std::min<size_t>((size_t)i - 1, h->temp_host.size() - 1)] == 1.0;
  if (temps_one && it >= cc->miniters) {
    if (m < st->best_MAP_metric) { st->best_MAP_metric = m; st->best_iter = it; st->inarow_no_best = 0; }
    else st->inarow_no_best += 1;
    if (st->inarow_no_change >= cc->Ninarow_nochange) { st->converged = 1; st->why = 1; }
    else if (st->inarow_no_best >= cc->Ninarow_nobest) { st->converged = 1; st->why = 2; }
    else if (it >= cc->maxiters) { st->converged = 1; st->why = 3; }
  }
  mr[12] = pc; mr[13] = st->inarow_no_change; mr[14] = st->inarow_no_best; mr[15] = st->inarow_na; mr[16] = st->converged;
  return 0;
}

// The sampling loop up to convergence as ONE call: blocks of iterations up to the next MAP check, get_MAP_ on the device,
// update_MAP_metrics_ (R/utils.R:356-397) and check_convergence_ (R/convergence.R:60-154) here on the host side of the ABI.
int bnmf_run_until(bnmf_handle* h, const bnmf_convergence_control* cc, bnmf_convergence_state* st, double* metrics, int cap_rows,
                   int* n_rows, double* map_rows, int cap_checks, int* n_checks) {
  if (!h || !cc || !st || !metrics || !n_rows || !map_rows || !n_checks) return fail(BNMF_EINVAL, "bnmf_run_until: null argument");
  if (!h->inited) return fail(BNMF_ESTATE, "bnmf_run_until: call bnmf_init first");
  if (h->cfg.window < cc->MAP_over) return fail(BNMF_ESTATE, "bnmf_run_until: the handle keeps %d samples, MAP_over = %d", h->cfg.window, cc->MAP_over);
  if (cc->MAP_every < 1 || cc->MAP_over < 1 || cc->metric < 0 || cc->metric > 4) return fail(BNMF_EINVAL, "bnmf_run_until: bad convergence control");
  const int N = h->cfg.N;
  *n_rows = 0; *n_checks = 0;
  std::vector<double> Am(N);
  std::vector<int32_t> used(cc->MAP_over);
  Timer tm{h, false};
  while (!st->converged && h->iter < cc->maxiters) {      // R/bayesNMF_sampler.R:268
    const int it0 = h->iter;
    int nxt = (it0 / cc->MAP_every + 1) * cc->MAP_every;
    if (nxt > cc->maxiters) nxt = cc->maxiters;
    const int n = nxt - it0;
    if (*n_rows + n > cap_rows) return fail(BNMF_ESIZE, "bnmf_run_until: metrics buffer too small (%d rows)", cap_rows);
    if (int rc = run_impl(h, n, 0, metrics + (size_t)*n_rows * BNMF_NMETRIC, tm)) return rc;
    const double* lastrow = metrics + (size_t)(*n_rows + n - 1) * BNMF_NMETRIC;
    *n_rows += n;
    const int it = h->iter;
    const int over = cc->MAP_over > cc->MAP_every ? cc->MAP_over : cc->MAP_every;
    if (!((it % cc->MAP_every == 0 && it >= over) || it >= cc->maxiters)) continue;      // :288-296
    if (*n_checks >= cap_checks) return fail(BNMF_ESIZE, "bnmf_run_until: MAP-metrics buffer too small (%d rows)", cap_checks);
    if (int rc = map_check(h, cc, st, lastrow, map_rows + (size_t)*n_checks * BNMF_NMAPROW, Am, used)) return rc;
    *n_checks += 1; st->n_checks += 1;
  }
  return 0;
}

// The post-warm-up tail of the MH models as ONE call (R/bayesNMF_sampler.R:332-384): post_warmup more iterations with
// state$converged = TRUE (true accept / reject), a MAP check whenever iter is a multiple of MAP_every and after the last one.
int bnmf_run_post_warmup(bnmf_handle* h, const bnmf_convergence_control* cc, bnmf_convergence_state* st, int post_warmup,
                         double* metrics, int cap_rows, int* n_rows, double* map_rows, int cap_checks, int* n_checks) {
  if (!h || !cc || !st || !metrics || !n_rows || !map_rows || !n_checks) return fail(BNMF_EINVAL, "bnmf_run_post_warmup: null argument");
  if (!h->inited) return fail(BNMF_ESTATE, "bnmf_run_post_warmup: call bnmf_init first");
  if (post_warmup < 0) return fail(BNMF_EINVAL, "bnmf_run_post_warmup: post_warmup < 0");
  if (h->cfg.window < cc->MAP_over) return fail(BNMF_ESTATE, "bnmf_run_post_warmup: the handle keeps %d samples, MAP_over = %d", h->cfg.window, cc->MAP_over);
  if (cc->MAP_every < 1 || cc->MAP_over < 1 || cc->metric < 0 || cc->metric > 4) return fail(BNMF_EINVAL, "bnmf_run_post_warmup: bad convergence control");
  *n_rows = 0; *n_checks = 0;
  std::vector<double> Am(h->cfg.N);
  std::vector<int32_t> used(cc->MAP_over);
  Timer tm{h, false};
  int done = 0;
  while (done < post_warmup) {
    const int it0 = h->iter;
    const int nxt = (it0 / cc->MAP_every + 1) * cc->MAP_every;
    const int n = std::min(nxt - it0, post_warmup - done);
    if (*n_rows + n > cap_rows) return fail(BNMF_ESIZE, "bnmf_run_post_warmup: metrics buffer too small (%d rows)", cap_rows);
    if (int rc = run_impl(h, n, 1, metrics + (size_t)*n_rows * BNMF_NMETRIC, tm)) return rc;
    const double* lastrow = metrics + (size_t)(*n_rows + n - 1) * BNMF_NMETRIC;
    *n_rows += n; done += n;
    if (!(h->iter % cc->MAP_every == 0 || done == post_warmup)) continue;
    if (*n_checks >= cap_checks) return fail(BNMF_ESIZE, "bnmf_run_post_warmup: MAP-metrics buffer too small (%d rows)", cap_checks);
    if (int rc = map_check(h, cc, st, lastrow, map_rows + (size_t)*n_checks * BNMF_NMAPROW, Am, used)) return rc;
    *n_checks += 1; st->n_checks += 1;
  }
  return 0;
}

// ---- measured ceilings for bench.py's roofline: Philox4x32-7 words per second (the count-allocation stream's generator) with
// nothing else in the loop (the floor of any allocation kernel: one word per count), and the device-to-device copy bandwidth ----
__global__ __launch_bounds__(256) void k_ubench_philox(uint32_t* out, int blocks_per_lane, uint32_t seed) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t acc = 0;
  for (int q = 0; q < blocks_per_lane; ++q) {
    const u32x4 w = philox4x32_7((uint32_t)q, gid, seed, 5u, 17u, 29u);
    acc += w.x ^ w.y ^ w.z ^ w.w;
  }
  out[gid] = acc;
}
int bnmf_ubench(int device, double* philox_words_per_s, double* copy_gbs) {
  if (!philox_words_per_s || !copy_gbs) return fail(BNMF_EINVAL, "bnmf_ubench: null argument");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  {
    const int wgs = prop.multiProcessorCount * 8, nq = 4000;                 // 8 waves per SIMD
    uint32_t* d = nullptr;
    HIPCHK(dmalloc(&d, (size_t)wgs * 256 * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_ubench_philox, dim3(wgs), dim3(256), 0, 0, d, 200, 1u);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_ubench_philox, dim3(wgs), dim3(256), 0, 0, d, nq, 1u);
    HIPCHK(hipEventRecord(e1, 0));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *philox_words_per_s = 4.0 * nq * (double)wgs * 256.0 / (ms * 1e-3);
    dfree(d);
  }
  {
    const size_t bytes = (size_t)1 << 30;
    char *a = nullptr, *b = nullptr;
    HIPCHK(dmalloc(&a, bytes)); HIPCHK(dmalloc(&b, bytes));
    HIPCHK(hipMemset(a, 1, bytes));
    HIPCHK(hipMemcpy(b, a, bytes, hipMemcpyDeviceToDevice));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(e0, 0));
    for (int r = 0; r < 4; ++r) HIPCHK(hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, 0));
    HIPCHK(hipEventRecord(e1, 0));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *copy_gbs = 4.0 * 2.0 * (double)bytes / (ms * 1e-3) / 1e9;               // read + write
    dfree(a); dfree(b);
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  return 0;
}

// ---- device-side probes for the parity tests ----
int bnmf_test_math(int device, int fn, const double* in, double* out, size_t n) {
  HIPCHK(hipSetDevice(device));
  double *di, *dou;
  HIPCHK(dmalloc(&di, n * sizeof(double)));
  HIPCHK(dmalloc(&dou, n * sizeof(double)));
  HIPCHK(hipMemcpy(di, in, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_test_math, dim3((n + 255) / 256), dim3(256), 0, 0, fn, di, dou, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dou, n * sizeof(double), hipMemcpyDeviceToHost));
  dfree(di); dfree(dou);
  return 0;
}
int bnmf_test_sampler(int device, int which, uint64_t seed, uint32_t chain, uint32_t var, uint32_t elem0, uint32_t iter,
                      const double* a, const double* b, const double* c, double* out, size_t n) {
  HIPCHK(hipSetDevice(device));
  if (which == 8) {                                 // rpois(a): k_test_rpois
    if (!a || !out) return fail(BNMF_EINVAL, "bnmf_test_sampler: probe 8 needs a and out");
    double *da8, *do8;
    HIPCHK(dmalloc(&da8, n * sizeof(double))); HIPCHK(dmalloc(&do8, n * sizeof(double)));
    HIPCHK(hipMemcpy(da8, a, n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_rpois, dim3((n + 255) / 256), dim3(256), 0, 0, (uint32_t)seed, (uint32_t)(seed >> 32) ^ chain, var, elem0, iter,
                       (const double*)da8, do8, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, do8, n * sizeof(double), hipMemcpyDeviceToHost));
    dfree(da8); dfree(do8);
    return 0;
  }
  if (int rc = ensure_alut(device)) return rc;
  double *da, *db, *dc, *dou;
  HIPCHK(dmalloc(&da, n * sizeof(double))); HIPCHK(dmalloc(&db, n * sizeof(double)));
  HIPCHK(dmalloc(&dc, n * sizeof(double))); HIPCHK(dmalloc(&dou, n * sizeof(double)));
  std::vector<double> zeros(n, 0.0);
  HIPCHK(hipMemcpy(da, a ? a : zeros.data(), n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db, b ? b : zeros.data(), n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dc, c ? c : zeros.data(), n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_test_sampler, dim3((n + 255) / 256), dim3(256), 0, 0, which, (uint32_t)seed, (uint32_t)(seed >> 32) ^ chain,
                     var, elem0, iter, da, db, dc, dou, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dou, n * sizeof(double), hipMemcpyDeviceToHost));
  dfree(da); dfree(db); dfree(dc); dfree(dou);
  return 0;
}
static int test_philox_r(int device, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4], int rounds) {
  HIPCHK(hipSetDevice(device));
  uint32_t* d;
  HIPCHK(dmalloc(&d, 16));
  hipLaunchKernelGGL(k_test_philox, dim3(1), dim3(1), 0, 0, ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], d, rounds);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, d, 16, hipMemcpyDeviceToHost));
  dfree(d);
  return 0;
}
int bnmf_test_philox(int device, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) { return test_philox_r(device, ctr, key, out, 10); }
int bnmf_test_philox7(int device, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) { return test_philox_r(device, ctr, key, out, 7); }

}  // extern "C"

#include "state_io.h"
