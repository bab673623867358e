// bayesnmf_amd/csrc/sweep.h — the scheduler: which kernel of an iteration goes on which of the handle's three streams, and how the hyper
// sweep of iteration t + 1 is handed to the draws of t + 1 (an in-kernel poll of a flag, the allocation kernel's gate, or a stream wait
// on an event).  Host code only, included by api.hip (one translation unit) between the handle's accessors and bnmf_init.
// The state the sweeps hand to each other is `h->pipe` (struct Pipe, api.hip, above bnmf_handle): its fields, writers, readers and
// invariants are stated there.  The host asserts below are live in the product build (it does not define NDEBUG).
#include <cassert>

// ------------------------------------------------------------------ launch helpers
static int need_hyper(bnmf_handle* h, std::initializer_list<int> ids) {
  for (int id : ids) if (!h->arr[id].d) return fail(BNMF_EUNSET, "hyper-prior array id %d was not set (fill_hyperprior_params, R/setup.R:15-88)", id);
  return 0;
}
static int ensure_metrics(bnmf_handle* h, size_t rows) {
  if (rows <= h->metrics_rows) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipHostFree(h->hMetrics));
  h->hMetrics = nullptr; h->dMetrics = nullptr;
  h->metrics_rows = rows;
  HIPCHK(hipHostMalloc((void**)&h->hMetrics, rows * BNMF_NMETRIC * sizeof(double), hipHostMallocMapped));
  HIPCHK(hipHostGetDevicePointer((void**)&h->dMetrics, h->hMetrics, 0));
  HIPCHK(hfree(h, h->dRaw));
  HIPCHK(hmalloc(h, &h->dRaw, rows * 8 * sizeof(double)));
  refresh_dev(h);
  return 0;
}
// Per-iteration partial sums (per-column metric terms, log-prior partials, MH acceptance partials) live in
// three slots (t % 3): k_reduce of iteration t is issued during iteration t+1 (see launch_side / launch_side_E), and the
// next writers of its slot are the kernels of iteration t+3.  Fixed-rank sweep: k_reduce(t) sits on side2 in front of
// Esum(t+2), whose flag releases k_pdraw(t+2) and with it everything of iteration t+2 and later on the main stream; the
// log-prior workgroups of side2 follow it in stream order.  Other sweeps: through ev_side (main stream) and ev_red (side2).
static void set_slot(const bnmf_handle* h, Dev& d, uint32_t t) {
  const size_t sl = t % 3u, G = h->cfg.G, N = h->cfg.N;
  d.colsse = h->dcol + sl * 3 * G; d.colll = d.colsse + G; d.colkl = d.colsse + 2 * G;
  d.lpE_part = h->dlpE + sl * (size_t)h->nblkE;
  d.lpPn = h->dlpPn + sl * N;
}
static void use_slot(bnmf_handle* h, uint32_t t) { set_slot(h, h->dev, t); }
static double* accPn_slot(const bnmf_handle* h, uint32_t t) { return h->mh.dAccPn ? h->mh.dAccPn + (size_t)(t % 3u) * h->cfg.N : nullptr; }
static double* accEp_slot(const bnmf_handle* h, uint32_t t) { return h->mh.dAccEpart ? h->mh.dAccEpart + (size_t)(t % 3u) * h->nblkE : nullptr; }
struct Timer {   // optional per-kernel HIP-event bracketing (serialises the two streams: profile mode only)
  bnmf_handle* h; bool on; double acc[BNMF_NKERNEL]{}; int cnt[BNMF_NKERNEL]{};
  void begin(int k, hipStream_t st) { if (on) { hipStreamSynchronize(h->stream); hipStreamSynchronize(h->side); hipStreamSynchronize(h->side2); hipEventRecord(h->ev[2 * k], st); } }
  void end(int k, hipStream_t st) { if (on) { hipEventRecord(h->ev[2 * k + 1], st); hipEventSynchronize(h->ev[2 * k + 1]); float ms = 0; hipEventElapsedTime(&ms, h->ev[2 * k], h->ev[2 * k + 1]); acc[k] += ms; cnt[k]++; } }
};
static RecDst rec_at(const bnmf_handle* h, uint32_t t, bool on);
static bool fused_rec(const bnmf_handle* h);
static double* ring_at(const bnmf_handle* h, int id, uint32_t t);
static RecDst rec_pdraw(const bnmf_handle* h, uint32_t t, bool on) {   // what k_pdraw records
  RecDst r = rec_at(h, t, on);
  if (h->cfg.learning_rank) { r.A = nullptr; r.R = nullptr; }          // then k_sumA records them, after the rank update
  return r;
}
// workgroups of the hyper sweep's P part (K N elements) and E part (N G elements), RT lanes each
static int side_nbP(const bnmf_handle* h) { return (int)(((size_t)h->cfg.K * h->cfg.N + RT - 1) / RT); }
static int side_nbE(const bnmf_handle* h) { return (int)(((size_t)h->cfg.N * h->cfg.G + RT - 1) / RT); }
static void launch_pdraw(bnmf_handle* h, uint32_t t, int from_prior, bool rec, const int* keep = nullptr) {   // keep: see k_pdraw
  const size_t lds = 2 * (size_t)h->cfg.K * sizeof(double);
  hipLaunchKernelGGL(k_pdraw, dim3(h->cfg.N), dim3(PD_T), lds, h->stream, h->dev, t, from_prior, 1, rec_pdraw(h, t, rec), SideWait{}, keep);
}
static void launch_edraw(bnmf_handle* h, uint32_t t, int from_prior, bool rec) {
  hipLaunchKernelGGL(k_edraw, dim3(h->nblkE), dim3(ES_T), 0, h->stream, h->dev, t, from_prior, 1, rec_at(h, t, rec).E);
}
// k_side for iteration t (reads P_{t-1}, E_{t-1}): issued on the side stream right after the draws
// of iteration t-1, so that it overlaps k_zalloc of iteration t-1
// tests (BNMF_DEBUG_ALLSIDE_DELAY_US): hold a side stream back in front of its next kernel — whatever then reads too early or writes too early shows
// as a bit that differs from the oracle's
static void dbg_delay(bnmf_handle* h, hipStream_t st) {
  if (h->dbg_allside_delay_us && st != h->stream) hipLaunchKernelGGL(k_debug_delay, dim3(1), dim3(64), 0, st, h->dbg_allside_delay_us);
}
// ... and the other way round (BNMF_DEBUG_MAIN_DELAY_US): the main stream held back, so that a side-stream kernel that runs on the main stream's
// results without waiting for them reads the values of the iteration before
static void dbg_delay_main(bnmf_handle* h) {
  if (h->dbg_main_delay_us) hipLaunchKernelGGL(k_debug_delay, dim3(1), dim3(64), 0, h->stream, h->dbg_main_delay_us);
}
// k_reduce of the iteration before, if launch_reduce left it pending, on stream st
static void issue_pending_reduce(bnmf_handle* h, Timer& tm, hipStream_t st) {
  if (!h->pipe.red_pending) return;
  const uint32_t t = h->pipe.red_t;
  h->pipe.red_pending = false;
  dbg_delay(h, st);
  Dev dr = h->dev;
  set_slot(h, dr, t);
  tm.begin(KN_REDUCE, st);
  hipLaunchKernelGGL(k_reduce, dim3(h->cfg.MH ? 5 : 4), dim3(RT), 0, st, dr, h->pipe.red_row, h->nblkE, (const double*)accPn_slot(h, t), (const double*)accEp_slot(h, t));
  tm.end(KN_REDUCE, st);
  // k_lpp's workgroups (side2) rewrite an lpPn slot this kernel read three iterations earlier: side2 waits for ev_red, unless the
  // reduce was issued on side2 itself (the fixed-rank sweep), where stream order does it without two runtime calls
  h->pipe.red_on_side2 = st == h->side2;
  if (!h->pipe.red_on_side2) { hipEventRecord(h->ev_red, st); h->pipe.red_issued = true; }
}
// ... or as workgroups of a kernel of the MH sweeps (k_mh_tail, the hosted column sweep): the slots they reduce; on = 0 if nothing is pending
static RedSlots take_reduce_slots(bnmf_handle* h) {
  if (!h->pipe.red_pending) return RedSlots{};
  const uint32_t t = h->pipe.red_t;
  Dev dr = h->dev;
  set_slot(h, dr, t);
  h->pipe.red_pending = false;
  return RedSlots{dr.colsse, dr.colll, dr.colkl, dr.lpE_part, dr.lpPn, accPn_slot(h, t), accEp_slot(h, t), h->pipe.red_row, 1};
}
// The per-column metric terms of iteration t from the Mhat k_zalloc_sort left (colterms.h), into the iteration's slot of the partial sums
static CtArgs ct_args(const bnmf_handle* h, uint32_t t) {
  const size_t G = h->cfg.G;
  double* sse = h->dcol + (size_t)(t % 3u) * 3 * G;
  return CtArgs{h->zs.dMh + (size_t)(t % 3u) * h->cfg.K * G, h->dev.M, h->dev.lgfact, h->dev.logm, sse, sse + G, sse + 2 * G, h->cfg.K, h->cfg.G, h->dev.maxM};
}
// The pending column terms, taken by the launch that will sum them: its arguments and n_ct workgroups (two columns per wavefront; k_colterms
// and k_side_lp's extra workgroups have the same shape).  Nothing pending: CtArgs{}, 0.
static_assert(CT_T == RT, "k_colterms and the column-term workgroups of k_side_lp share one grid size");
static CtArgs take_colterms(bnmf_handle* h, int& n_ct) {
  n_ct = 0;
  if (!h->pipe.ct_pending) return CtArgs{};
  const CtArgs a = ct_args(h, h->pipe.ct_pending);
  n_ct = (h->cfg.G + 2 * (RT / 64) - 1) / (2 * (RT / 64));
  h->pipe.ct_pending = 0;
  return a;
}
// ... as a launch of its own on the main stream (behind the allocation kernel in stream order): whenever the next kernel on that stream
// is not a merged draw kernel that could take the work along (first sweeps of a chain, two-kernel sweep, profile mode, end of a call)
static void flush_colterms(bnmf_handle* h) {
  int n_ct = 0;
  const CtArgs a = take_colterms(h, n_ct);
  if (n_ct) hipLaunchKernelGGL(k_colterms, dim3((unsigned)n_ct), dim3(CT_T), 0, h->stream, a);
}
// ev_sideP (side2 done) and ev_side (side done, behind ev_sideP) are what a main-stream wait or flush_reduce needs; in the
// steady state of the fixed-rank sweep nobody waits for them (k_pdraw polls flags), so they are recorded on demand: a later
// record covers everything enqueued before it
static void chain_ev_side(bnmf_handle* h) {       // ev_side behind an ev_sideP that has just been recorded on side2
  hipStreamWaitEvent(h->side, h->ev_sideP, 0);
  hipEventRecord(h->ev_side, h->side);
  h->pipe.side_ev_stale = false;
}
static void record_side_events(bnmf_handle* h) { hipEventRecord(h->ev_sideP, h->side2); chain_ev_side(h); }
static void refresh_side_events(bnmf_handle* h) { if (h->pipe.side_ev_stale) record_side_events(h); }
static void launch_side(bnmf_handle* h, uint32_t t, Timer& tm, bool publish = false) {
  const int nbP = side_nbP(h), nbE = side_nbE(h);
  hipEventRecord(h->ev_draw, h->stream);
  hipStreamWaitEvent(h->side, h->ev_draw, 0);
  tm.begin(KN_SIDE, h->side);
  // publish (MH / Normal sweeps): the last workgroup raises flag [1] = t, which the next P-row kernel polls (no barrier packet)
  dbg_delay(h, h->side);
  hipLaunchKernelGGL(k_side, dim3(h->cfg.N + nbP + nbE), dim3(RT), 0, h->side, h->dev, t, nbP, 0, rec_at(h, t, fused_rec(h)),
                     publish ? SideDone{h->dFlags, h->dFlags + 1, (unsigned)(h->cfg.N + nbP + nbE), t} : SideDone{});
  h->pipe.flags_valid = publish;
  tm.end(KN_SIDE, h->side);
  hipEventRecord(h->ev_side, h->side);
  hipEventRecord(h->ev_sideP, h->side);
  h->pipe.side_ev_stale = false;
  h->pipe.side_valid = true;
  h->pipe.side_main = false;
  // k_reduce of the PREVIOUS iteration: its inputs are complete once the draws of this iteration have run
  // (main-stream order), which ev_draw above implies, so the main stream needs no marker after k_zalloc
  issue_pending_reduce(h, tm, h->side);
}
// MH / Normal sweeps, steady state (round 4): the hyper sweep of iteration t on the MAIN stream, between the column kernel of t-1 and
// its tail kernel.  On the side stream it was released by the column kernel through an event (12 us late), ran 20 us beside a 12 us tail
// kernel, and the next P-row kernel waited 13.6 us of its 101 for the flag (profiles/r04_cfg3_kernel_stats.csv, r04_mh_prow_stamps.txt);
// alone on the device it is shorter than that wait, and the row kernel behind it needs neither flag nor event.
static void launch_side_main(bnmf_handle* h, uint32_t t, Timer& tm) {
  const int nbP = side_nbP(h), nbE = side_nbE(h);
  tm.begin(KN_SIDE, h->stream);
  hipLaunchKernelGGL(k_side, dim3(h->cfg.N + nbP + nbE), dim3(RT), 0, h->stream, h->dev, t, nbP, 0, rec_at(h, t, fused_rec(h)), SideDone{});
  tm.end(KN_SIDE, h->stream);
  h->pipe.flags_valid = false;
  h->pipe.side_valid = true;
  h->pipe.side_main = true;
  // (k_reduce of the PREVIOUS iteration: inside this iteration's k_mh_tail, see launch_mh_metrics)
}
// The same work in three launches, for the Gibbs sweep.  The P-side hyper sweep depends on P_{t-1} only and has
// the longest per-lane latency (rejection sampling of Alpha): it starts right behind k_pdraw on its own stream.
// Esum follows it once k_edraw is done; both are over long before k_zalloc, so that the event the next k_pdraw
// waits for is already satisfied when the main stream reaches it (a late cross-stream event costs ~12 us).
// The E-side sweep (needed only by the next k_edraw) shares the CUs with k_zalloc and ends with it.
// what k_lpe reads as E_t: the ring slot of iteration t when the sweep records (safe for a whole window), else the live E
// (then sweep() double-buffers E)
static bool lpe_from_ring(const bnmf_handle* h) { return fused_rec(h) && h->arr[BNMF_E].ring != nullptr; }
static const double* lpe_src(const bnmf_handle* h, uint32_t t) { return lpe_from_ring(h) ? ring_at(h, BNMF_E, t) : h->dev.E; }
static void launch_side_P(bnmf_handle* h, uint32_t t) {   // ev_p = completion of k_pdraw(t-1)
  const int nbP = side_nbP(h);
  hipStreamWaitEvent(h->side2, h->ev_p, 0);
  // k_lpp below rewrites lpPn slot (t-1) % 3, last read by k_reduce of iteration t-4 (side stream): order behind it
  if (h->pipe.red_issued && !h->pipe.red_on_side2) hipStreamWaitEvent(h->side2, h->ev_red, 0);
  // ... and the log-prior of the P just drawn (k_lpp's work, iteration t-1) in the same launch
  dbg_delay(h, h->side2);
  hipLaunchKernelGGL(k_side_lp, dim3(nbP + h->cfg.N), dim3(RT), 0, h->side2, h->dev, t, nbP, h->cfg.N, rec_at(h, t, fused_rec(h)), SideDone{},
                     SideExtra{nbP, h->cfg.N, 0, t - 1, nullptr, 0}, CtArgs{});
}
static void launch_side_E(bnmf_handle* h, uint32_t t, Timer& tm, bool e_done = false) {   // ev_draw = completion of k_edraw(t-1); e_done: k_draw ran the E-side sweep
  const int nbP = side_nbP(h), nbE = side_nbE(h);
  hipStreamWaitEvent(h->side2, h->ev_draw, 0);
  // Esum closes the side2 work the next k_pdraw needs (the P part ran before it on the same stream): it publishes flag [3]
  // ... and, in the same launch, the log-prior of the E just drawn (k_lpe's work; iteration t-1, whose slot pointers h->dev
  // still holds): off the critical path
  dbg_delay(h, h->side2);
  // (the per-column metric terms of the iteration before ride along as in launch_side_merged: workgroups behind the log-prior ones)
  int n_ct = 0;
  const CtArgs ct = take_colterms(h, n_ct);
  hipLaunchKernelGGL(k_side_lp, dim3(h->cfg.N + h->nblkE + n_ct), dim3(RT), 0, h->side2, h->dev, t, nbP, 0, RecDst{}, SideDone{h->dFlags + 2, h->dFlags + 3, (unsigned)(h->cfg.N + h->nblkE), t},
                     SideExtra{h->cfg.N, 0, h->nblkE, t - 1, lpe_src(h, t - 1), 1}, ct);
  // k_reduce of the PREVIOUS iteration here, behind the kernels that produce its inputs on this stream (k_lpp, k_lpe) and
  // behind ev_draw (k_zalloc of that iteration): on the E part's stream it sat in front of the next E-side sweep, and the
  // P part waited for its event
  issue_pending_reduce(h, tm, h->side2);
  if (!e_done) {
    hipStreamWaitEvent(h->side, h->ev_draw, 0);
    dbg_delay(h, h->side);
    hipLaunchKernelGGL(k_side, dim3(nbE), dim3(RT), 0, h->side, h->dev, t, nbP, h->cfg.N + nbP, rec_at(h, t, fused_rec(h)), SideDone{h->dFlags, h->dFlags + 1, (unsigned)nbE, t});
  }
  h->pipe.flags_valid = true;
  // ev_side (the E part AND the P part / Esum / log-priors done) for a main-stream wait: on demand, see refresh_side_events
  h->pipe.side_ev_stale = true;
  h->pipe.side_valid = true;
}
// Behind the merged draw kernel (which runs the E-side sweep itself): the P-side hyper sweep of iteration t on `side`, with a
// flag of its own ([9]); Esum(t) and the log-priors of iteration t-1 in ONE launch on side2 (flag [3] counts all its
// workgroups), k_reduce behind it.  The two no longer share a stream: the P-side sweep is a few long per-lane chains and
// held Esum's flag back.
static void launch_side_merged(bnmf_handle* h, uint32_t t, Timer& tm) {
  const int N = h->cfg.N;
  const int nbP = side_nbP(h);
  hipStreamWaitEvent(h->side, h->ev_draw, 0);
  if (h->dbg_side_delay_us) hipLaunchKernelGGL(k_debug_delay, dim3(1), dim3(64), 0, h->side, h->dbg_side_delay_us);   // tests: a late P-side sweep
  dbg_delay(h, h->side);
  hipLaunchKernelGGL(k_side, dim3(nbP), dim3(RT), 0, h->side, h->dev, t, nbP, N, rec_at(h, t, fused_rec(h)), SideDone{h->dFlags + 8, h->dFlags + 9, (unsigned)nbP, t});
  // (Round 5, measured and NOT adopted: releasing the side streams by the draw kernel's flag — one polling wavefront at the head of each side
  // stream, P / E stored write-through, no stop event on the draw kernel.  The stop event costs ~6 us between the draw kernel's end and the
  // allocation kernel's start in the traces and its signal reaches the side queues 12-20 us later, differently from process to process
  // (tools/bimodal.sh: steady iteration 80.6 us in most processes, 83.3 us in about a quarter) — but with the flag the side kernels start
  // WITH the allocation kernel and take its issue slots from its first task on: 80.3 -> 96.4 us per iteration, bit-exact.)
  hipStreamWaitEvent(h->side2, h->ev_draw, 0);
  if (h->pipe.red_issued && !h->pipe.red_on_side2) hipStreamWaitEvent(h->side2, h->ev_red, 0);   // lpPn slot reuse, see launch_side_P
  dbg_delay(h, h->side2);
  // the per-column metric terms of iteration t - 2 ride along (its allocation kernel ran before the draw kernel whose stop event this stream
  // has just waited for): extra workgroups behind the log-prior ones, beside the allocation kernel of t - 1; k_reduce(t - 2) follows below
  int n_ct = 0;
  const CtArgs ct = take_colterms(h, n_ct);
  hipLaunchKernelGGL(k_side_lp, dim3(2 * N + h->nblkE + n_ct), dim3(RT), 0, h->side2, h->dev, t, nbP, 0, RecDst{}, SideDone{h->dFlags + 2, h->dFlags + 3, (unsigned)(2 * N + h->nblkE), t},
                     SideExtra{N, N, h->nblkE, t - 1, lpe_src(h, t - 1), 1}, ct);
  issue_pending_reduce(h, tm, h->side2);
  h->pipe.flags_valid = true;
  h->pipe.side_ev_stale = true;
  h->pipe.side_valid = true;
  h->pipe.gate_f0 = 9;
}
// Rank learning: the hyper sweep of t+1 in two parts.  Early (released by k_edraw): the k_side kernels.  They hold 64+ VGPRs
// and cannot be scheduled on a CU whose SIMDs carry two waves of the rank sweep (230 VGPRs each): they run on the ~100 CUs
// the rank sweep leaves free and are done before k_zalloc starts.  Late (released by the rank sweep): the small log-prior
// kernels (16-28 VGPRs), which DO fit beside rank-sweep waves and delayed the whole co-resident grid at every factor, and
// Esum, whose flag releases the next iteration's draws and therefore has to come after them.
static void launch_side_early(bnmf_handle* h, uint32_t t) {
  const int nbP = side_nbP(h), nbE = side_nbE(h);
  hipStreamWaitEvent(h->side2, h->ev_draw, 0);
  dbg_delay(h, h->side2);
  hipLaunchKernelGGL(k_side, dim3(nbP), dim3(RT), 0, h->side2, h->dev, t, nbP, h->cfg.N, rec_at(h, t, fused_rec(h)), SideDone{});
  // Esum of t needs E only: summed here, beside the rank sweep (end of round 5).  Behind the rank sweep — where its flag has to be raised, see
  // launch_side_late — its 50 workgroups sat beside the allocation kernel for 121 us of a 10 us reduction, and the next k_pdraw polled for them
  dbg_delay(h, h->side2);
  hipLaunchKernelGGL(k_side, dim3(h->cfg.N), dim3(RT), 0, h->side2, h->dev, t, nbP, 0, RecDst{}, SideDone{});
  hipStreamWaitEvent(h->side, h->ev_draw, 0);
  dbg_delay(h, h->side);
  hipLaunchKernelGGL(k_side, dim3(nbE), dim3(RT), 0, h->side, h->dev, t, nbP, h->cfg.N + nbP, rec_at(h, t, fused_rec(h)), SideDone{h->dFlags, h->dFlags + 1, (unsigned)nbE, t});
  h->pipe.flags_valid = true;
}
static void launch_side_late(bnmf_handle* h, uint32_t t, Timer& tm) {
  hipStreamWaitEvent(h->side2, h->ev_rank, 0);
  // k_lpp rewrites lpPn slot (t-1) % 3, last read by k_reduce of iteration t-4 (side stream): order behind it
  if (h->pipe.red_issued) hipStreamWaitEvent(h->side2, h->ev_red, 0);
  dbg_delay(h, h->side2);
  hipLaunchKernelGGL(k_lpp, dim3(h->cfg.N), dim3(64), 0, h->side2, h->dev, t - 1);   // log-prior of the P just drawn
  dbg_delay(h, h->side2);
  hipLaunchKernelGGL(k_lpe, dim3(h->nblkE), dim3(ES_T), 0, h->side2, h->dev, t - 1, lpe_src(h, t - 1)); // ... and of the E just drawn
  // Esum's flag [3] last: it releases the next iteration's draws, which overwrite the P and E the two kernels above read (the sums
  // themselves were made by launch_side_early on this stream)
  dbg_delay(h, h->side2);
  hipLaunchKernelGGL(k_raise_flag, dim3(1), dim3(64), 0, h->side2, h->dFlags + 3, t);
  record_side_events(h);                                   // (never stale here: the rank-learning sweep records them every iteration)
  h->pipe.side_valid = true;
  issue_pending_reduce(h, tm, h->side);
}
// once per handle and allocation kernel (a handle launches one): allow > 64 KiB of dynamic LDS
static int raise_lds_limit(bnmf_handle* h, const void* kern) {
  if (h->z_attr_kernel == kern) return 0;
  HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  h->z_attr_kernel = kern;
  return 0;
}
template <typename KernelT, typename ArgT>
static int launch_z(bnmf_handle* h, uint32_t t, KernelT kern, const ArgT& arg, int zt) {
  if (int rc = raise_lds_limit(h, (const void*)kern)) return rc;
  hipLaunchKernelGGL(kern, dim3(h->zw.grid), dim3(zt), h->zw.lds, h->stream, arg, t, h->zw.g, h->z_ablate);
  return 0;
}
static ZArgs zargs(const bnmf_handle* h) {
  const Dev& d = h->dev;
  ZArgs za{d.K, d.G, d.N, d.maxM, d.k0, d.k1, d.M, d.P, d.E, d.A, d.ZsumK, d.ZsumG, d.Z, d.colsse, d.colll, d.colkl, d.lgfact, d.logm, nullptr, nullptr, 0u, nullptr};
  if (h->pipe.z_gate_next) { za.gate0 = h->dFlags + h->pipe.gate_f0; za.gate1 = h->dFlags + 3; za.gate_epoch = h->pipe.z_gate_next; za.gate_err = h->dErr; }
  return za;
}
template <bool SZ, int ZT_, bool DIAG>
static int launch_zreg_t(bnmf_handle* h, uint32_t t) {
  const ZArgs za = zargs(h);
  switch (h->zw.g.TR) {
    case 8: return launch_z(h, t, k_zalloc_reg<SZ, ZT_, 8, DIAG>, za, ZT_);
    case 16: return launch_z(h, t, k_zalloc_reg<SZ, ZT_, 16, DIAG>, za, ZT_);
    case 20: return launch_z(h, t, k_zalloc_reg<SZ, ZT_, 20, DIAG>, za, ZT_);
    default: return launch_z(h, t, k_zalloc_reg<SZ, ZT_, 24, DIAG>, za, ZT_);
  }
}
template <bool SZ, int ZT_, bool LEAN_>
static int launch_ztile(bnmf_handle* h, uint32_t t) {
  auto kern = k_zalloc_tile<SZ, ZT_, LEAN_>;
  if (int rc = raise_lds_limit(h, (const void*)kern)) return rc;
  const ZArgs za = zargs(h);
  hipLaunchKernelGGL(kern, dim3(h->zt.grid), dim3(ZT_), h->zt.lds, h->stream, za, h->zt.dMhat, t, h->zt.g);
  hipLaunchKernelGGL(k_colmetrics<256>, dim3((h->cfg.G + 3) / 4), dim3(256), 0, h->stream, za, (const double*)h->zt.dMhat);
  if (h->zt.g.dbg) {                                        // BNMF_ZTDBG: section cycles (100 MHz s_memtime ticks) per launch
    unsigned long long v[8];
    hipStreamSynchronize(h->stream);
    hipMemcpy(v, h->zt.g.dbg, sizeof v, hipMemcpyDeviceToHost);
    hipMemset(h->zt.g.dbg, 0, sizeof v);
    if (v[0]) fprintf(stderr, "[ztile t=%u] waves %llu grid %d w %d lds %zu  per wave: phase1 %.1f  phase2 %.1f  flush %.1f  columns %.1f  kernel %.1f (s_memtime ticks)\n",
                      t, v[0], h->zt.grid, h->zt.w, h->zt.lds, (double)v[1] / v[0], (double)v[2] / v[0], (double)v[3] / v[0], (double)v[4] / v[0], (double)v[5] / v[0]);
  }
  return 0;
}
template <bool SZ, int ZT_>
static int launch_zalloc_t(bnmf_handle* h, uint32_t t) {
  if (h->zkind == ZKind::tile) return (h->zt.lean && ZT_ == 1024) ? launch_ztile<SZ, ZT_, (ZT_ == 1024)>(h, t) : launch_ztile<SZ, ZT_, false>(h, t);
  if (h->zkind == ZKind::general) return launch_z(h, t, k_zalloc<SZ, ZT_>, h->dev, ZT_);
#ifdef BNMF_DIAG
  if (h->z_ablate) return launch_zreg_t<SZ, ZT_, true>(h, t);   // the DIAG instantiation honours BNMF_ABLATE
#endif
  return launch_zreg_t<SZ, ZT_, false>(h, t);
}
static int zs_prio() { static const int v = getenv("BNMF_ZSPRIO") ? atoi(getenv("BNMF_ZSPRIO")) : 1; return v; }   // A/B: 0 = the allocation kernel at default issue priority
// where the item records of iteration t go (save_Z on the sorted schedule): the sample's slot of the record ring, or the one buffer
static uint32_t* zs_rec_at(const bnmf_handle* h, uint32_t t) {
  if (!h->zs.dRec) return nullptr;
  return h->zs.dRecRing ? h->zs.dRecRing + (size_t)((t - 1) % (uint32_t)h->wcap) * h->zs.recwords : h->zs.dRec;
}
// Z[k, n, g] of iteration t from its records into h->dZ (main stream)
static void launch_zexpand(bnmf_handle* h, uint32_t t) {
  const ZSArgs sa{zargs(h), h->zs.dItems, h->zs.dBlocks, h->zs.dCols, h->zs.dM, h->zs.it16, h->zs.qmax, zs_rec_at(h, t), nullptr, 0, 0, h->zs.dProf};
  hipLaunchKernelGGL(k_zexpand, dim3(h->zs.g.nblocks), dim3(ZX_T), h->zs.x_lds, h->stream, sa, h->zs.x_cols);
  h->pipe.z_expanded_iter = (int)t;
}
static int ensure_Z(bnmf_handle* h) {
  if (h->zkind != ZKind::sort || !h->zs.dRec || !h->cfg.save_Z || h->iter < 1 || h->pipe.z_expanded_iter == h->iter) return 0;
  HIPCHK(hipSetDevice(h->device));
  launch_zexpand(h, (uint32_t)h->iter);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
template <int ZT_>
static int launch_zsort_t(bnmf_handle* h, uint32_t t) {
  const ZSArgs sa{zargs(h), h->zs.dItems, h->zs.dBlocks, h->zs.dCols, h->zs.dM, h->zs.it16, h->zs.qmax, zs_rec_at(h, t), h->zs.dMh + (size_t)(t % 3u) * h->cfg.K * h->cfg.G, zs_prio(), h->zs.shared ? 1 : 0, h->zs.dProf};
  auto go = [&](auto kern) -> int {
    if (int rc = raise_lds_limit(h, (const void*)kern)) return rc;
    hipLaunchKernelGGL(kern, dim3(h->zs.g.nblocks), dim3(ZT_), h->zs.lds, h->stream, sa, t, h->zs.g);
    return 0;
  };
  // the geometry-fixed instantiations (zalloc_sort.h ZSFixed; chosen by build_zsort, BNMF_ZSFIXED=0: never): 14 waves, two factors per word,
  // raised issue priority, no record, no shared column.  Every other handle takes the dynamic form below, as before round 6.
  if constexpr (ZT_ == ZSFIX_ZT) {
    if (h->zs.fixed && sa.prio != 0 && !sa.rec && !sa.shared) switch (h->zs.fixed) {
      case 1: return go(k_zalloc_sort<ZSFIX_ZT, ZSFIX_NBLK, true, ZSFix10k>);
      case 2: return go(k_zalloc_sort<ZSFIX_ZT, ZSFIX_NBLK, true, ZSFix2k>);
      default: break;
    }
  }
#ifdef BNMF_FASTBUILD   /* builder's experiment builds only (one allocation kernel: the metric configuration's): never the product */
  if (h->zs.nblk != 4) return fail(BNMF_EMODEL, "BNMF_FASTBUILD: only N = 16..20");
  return h->zs.pk ? go(k_zalloc_sort<ZT_, 4, true>) : go(k_zalloc_sort<ZT_, 4, false>);
#else
  if (h->zs.pk) switch (h->zs.nblk) {
    case 1: return go(k_zalloc_sort<ZT_, 1, true>);
    case 2: return go(k_zalloc_sort<ZT_, 2, true>);
    case 3: return go(k_zalloc_sort<ZT_, 3, true>);
    case 4: return go(k_zalloc_sort<ZT_, 4, true>);
    default: return go(k_zalloc_sort<ZT_, 5, true>);
  }
  switch (h->zs.nblk) {
    case 1: return go(k_zalloc_sort<ZT_, 1, false>);
    case 2: return go(k_zalloc_sort<ZT_, 2, false>);
    case 3: return go(k_zalloc_sort<ZT_, 3, false>);
    case 4: return go(k_zalloc_sort<ZT_, 4, false>);
    default: return go(k_zalloc_sort<ZT_, 5, false>);
  }
#endif
}
static int launch_zsort(bnmf_handle* h, uint32_t t) {
#ifdef BNMF_FASTBUILD
  if (h->zs.w == 14) return launch_zsort_t<896>(h, t);
  if (h->zs.w != 12) return fail(BNMF_EMODEL, "BNMF_FASTBUILD: only 12 or 14 waves");
  return launch_zsort_t<768>(h, t);
#else
  switch (h->zs.w) {
    case 16: return launch_zsort_t<1024>(h, t);
    case 14: return launch_zsort_t<896>(h, t);
    case 12: return launch_zsort_t<768>(h, t);
    case 8: return launch_zsort_t<512>(h, t);
    case 6: return launch_zsort_t<384>(h, t);
    default: return launch_zsort_t<256>(h, t);
  }
#endif
}
static int launch_zstep(bnmf_handle* h, uint32_t t) {
  const ZPArgs pa{zargs(h), h->zp.dItems, h->zp.it16 ? 1 : 0, h->zp.dWgs, h->zp.dBatches, h->zp.dSteps, h->zp.dCols};
  auto go = [&](auto kern) -> int {
    if (int rc = raise_lds_limit(h, (const void*)kern)) return rc;
    hipLaunchKernelGGL(kern, dim3(h->zp.g.nwg), dim3(h->zp.ns * 64), h->zp.lds, h->stream, pa, t, h->zp.g);
    return 0;
  };
  return h->zp.gbp == 40 ? go(k_zalloc_step<4, 40, 8>) : go(k_zalloc_step<4, 32, 8>);
}
static int launch_zalloc(bnmf_handle* h, uint32_t t) {
  int w = 0;                                               // waves per workgroup of the three kernels instantiated by width
  switch (h->zkind) {
    case ZKind::none: return fail(BNMF_ESTATE, "launch_zalloc: the handle allocates no counts");
    case ZKind::sort:
      if (int rc = launch_zsort(h, t)) return rc;
      // save_Z: the items' records ARE the sample (zs_rec_at); Z is expanded from them when it is read (ensure_Z, bnmf_window)
      if (h->cfg.save_Z && h->zs.eager) launch_zexpand(h, t);
      return 0;
    case ZKind::step: return launch_zstep(h, t);
    case ZKind::tile: w = h->zt.w; break;
    case ZKind::reg: case ZKind::general: w = h->zw.w; break;
  }
  const bool sz = h->cfg.save_Z != 0;
#ifdef BNMF_FASTBUILD
  if (w != 16) return fail(BNMF_EMODEL, "BNMF_FASTBUILD: only 16 waves");
  return sz ? launch_zalloc_t<true, 1024>(h, t) : launch_zalloc_t<false, 1024>(h, t);
#else
  switch (w) {
    case 16: return sz ? launch_zalloc_t<true, 1024>(h, t) : launch_zalloc_t<false, 1024>(h, t);
    case 8: return sz ? launch_zalloc_t<true, 512>(h, t) : launch_zalloc_t<false, 512>(h, t);
    case 6: return sz ? launch_zalloc_t<true, 384>(h, t) : launch_zalloc_t<false, 384>(h, t);
    case 4: return sz ? launch_zalloc_t<true, 256>(h, t) : launch_zalloc_t<false, 256>(h, t);
    case 2: return sz ? launch_zalloc_t<true, 128>(h, t) : launch_zalloc_t<false, 128>(h, t);
    default: return sz ? launch_zalloc_t<true, 64>(h, t) : launch_zalloc_t<false, 64>(h, t);
  }
#endif
}
// sample_R then sample_An for n = 1..N (R/sample_params.R:67-74): one persistent launch for the N sequential updates
// row >= 0 (Gibbs sweep): the kernel also records A, R and sum(A) of the iteration (k_sumA's work)
static void launch_rank(bnmf_handle* h, uint32_t t, hipEvent_t stop = nullptr, int row = -1) {
  const int N = h->cfg.N;
  const int NB = (h->cfg.G + RK_MAXC - 1) / RK_MAXC;
  const size_t lds = (3 * (size_t)N + 1) * sizeof(double);            // A, sample_R weights, sample_An uniforms
  const RecDst rr = row >= 0 ? rec_at(h, t, fused_rec(h)) : RecDst{};
  auto go = [&](auto kern) {
    hipExtLaunchKernelGGL(kern, dim3(h->rank.grid), dim3(h->rank.half ? RK_TH : RK_T), (uint32_t)lds, h->stream, nullptr, stop, 0, h->dev, t, (unsigned long long*)h->rank.dCol, NB, h->dErr + 1, h->rank.dMhat, (unsigned long long*)h->rank.dDbg, row, rr.A, rr.R);
  };
  const bool nrm = h->cfg.likelihood == BNMF_NORMAL;
  if (h->rank.half) { if (nrm) go(k_rank_sweep<true, true, true>); else go(k_rank_sweep<true, false, true>); }
  else if (h->rank.reg) { if (nrm) go(k_rank_sweep<true, true>); else go(k_rank_sweep<true, false>); }
  else { if (nrm) go(k_rank_sweep<false, true>); else go(k_rank_sweep<false, false>); }
}
// ids recorded per iteration (names(self$params) + names(self$prior_params), R/bayesNMF_sampler.R:245-252)
static std::vector<int> recorded_ids(const bnmf_handle* h) {
  std::vector<int> ids = {BNMF_P, BNMF_E, BNMF_A, BNMF_R};
  if (h->cfg.prior == BNMF_GAMMA) ids.insert(ids.end(), {BNMF_ALPHA_P, BNMF_BETA_P, BNMF_ALPHA_E, BNMF_BETA_E});
  else if (h->cfg.prior == BNMF_EXPONENTIAL) ids.insert(ids.end(), {BNMF_LAMBDA_P, BNMF_LAMBDA_E});
  else ids.insert(ids.end(), {BNMF_MU_P, BNMF_SIGMASQ_P, BNMF_MU_E, BNMF_SIGMASQ_E});
  if (h->cfg.MH) ids.insert(ids.end(), {BNMF_ACC_P, BNMF_ACC_E});
  if (h->cfg.likelihood == BNMF_NORMAL) ids.push_back(BNMF_SIGMASQ);
  return ids;
}
static int ensure_rings(bnmf_handle* h) {
  if (h->cfg.window <= 0) return 0;
  h->wcap = h->cfg.window + 1;
  for (int id : recorded_ids(h)) {
    Arr& a = h->arr[id];
    if (!a.ring) if (int rc = ring_alloc(h->device, (size_t)h->wcap * id_len(h, id) * sizeof(double), &a.ring)) return rc;
  }
  const bool recs = h->zkind == ZKind::sort && h->zs.dRec;   // samples$Z on the sorted schedule: a ring of item records (zs_rec_at)
  if (h->dZ && !(recs ? (void*)h->zs.dRecRing : (void*)h->zring)) {   // else (R/bayesNMF_sampler.R:245-252) K*N*G ints per kept sample
    const size_t bytes = (size_t)h->wcap * (recs ? h->zs.recwords : id_len(h, BNMF_Z)) * 4;
    if ((double)bytes / 1e9 <= env_real("BNMF_ZRING_GB", 32.0)) HIPCHK(recs ? hmalloc(h, &h->zs.dRecRing, bytes) : hmalloc(h, &h->zring, bytes));
  }
  return 0;
}
static void record_Z(bnmf_handle* h, uint32_t t) {
  if (!h->zring) return;                                   // (sorted schedule: the allocation kernel wrote the sample's records into its ring slot)
  const size_t len = id_len(h, BNMF_Z);
  hipMemcpyAsync(h->zring + (size_t)((t - 1) % (uint32_t)h->wcap) * len, h->dZ, len * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream);
}
// the Gibbs sweep (Poisson, no MH) records inside its producers: k_pdraw (P, and A, R when the rank is fixed), k_edraw (E),
// k_side (prior parameters), k_sumA (A, R when the rank is learned).  The MH / Normal sweeps copy with k_record.
static bool fused_rec(const bnmf_handle* h) { return h->cfg.window > 0 && !h->cfg.MH && h->cfg.likelihood == BNMF_POISSON; }
static double* ring_at(const bnmf_handle* h, int id, uint32_t t) {
  const Arr& a = h->arr[id];
  return a.ring ? a.ring + (size_t)((t - 1) % (uint32_t)h->wcap) * id_len(h, id) : nullptr;
}
static RecDst rec_at(const bnmf_handle* h, uint32_t t, bool on) {
  RecDst r{};
  if (!on || h->wcap <= 0) return r;
  r.P = ring_at(h, BNMF_P, t); r.E = ring_at(h, BNMF_E, t); r.A = ring_at(h, BNMF_A, t); r.R = ring_at(h, BNMF_R, t);
  static const int PP[3][4] = {{BNMF_MU_P, BNMF_SIGMASQ_P, BNMF_MU_E, BNMF_SIGMASQ_E},      // indexed by the prior enum
                               {BNMF_LAMBDA_P, -1, BNMF_LAMBDA_E, -1},
                               {BNMF_ALPHA_P, BNMF_BETA_P, BNMF_ALPHA_E, BNMF_BETA_E}};
  const int* pp = PP[h->cfg.prior];
  for (int i = 0; i < 4; ++i) r.pp[i] = pp[i] >= 0 ? ring_at(h, pp[i], t) : nullptr;
  return r;
}
static int record_args(bnmf_handle* h, uint32_t t, RecArgs& ra) {
  ra = RecArgs{}; ra.n = 0; ra.R = nullptr; ra.Rdst = nullptr;
  const int W = h->cfg.window;
  if (W <= 0) return 0;
  const size_t slot = (size_t)((t - 1) % (uint32_t)h->wcap);
  for (int id : recorded_ids(h)) {
    Arr& a = h->arr[id];
    const size_t len = id_len(h, id);
    if (!a.ring) return fail(BNMF_ESTATE, "record: ring of id %d missing", id);
    if (id == BNMF_R) { ra.R = h->dR; ra.Rdst = a.ring + slot; continue; }
    if (!a.d) continue;
    ra.src[ra.n] = a.d + (is_prior_param(id) ? (size_t)(t & 1u) * len : 0);
    ra.dst[ra.n] = a.ring + slot * len;
    ra.len[ra.n] = len;
    ra.n++;
  }
  return 0;
}
static int launch_record(bnmf_handle* h, uint32_t t) {
  RecArgs ra;
  if (int rc = record_args(h, t, ra)) return rc;
  if (ra.n > 0 || ra.Rdst) hipLaunchKernelGGL(k_record, dim3(512), dim3(256), 0, h->stream, ra);
  return 0;
}
// k_reduce of iteration t: on the side stream, after the main stream has finished k_zalloc / metrics of t
// metrics of iteration t: sum(A) now (main stream, right after the rank update); the canonical reductions later
static void launch_reduce(bnmf_handle* h, uint32_t t, int row, Timer& tm, bool rank_wrote = false) {   // rank_wrote: k_rank_sweep recorded A, R, sum(A)
  // sum(A) and the A-masked acceptance sum (MH / Normal sweeps, init); the Gibbs sweep's rank kernel writes sum(A), A, R itself
  if (h->cfg.learning_rank && !rank_wrote) hipLaunchKernelGGL(k_sumA, dim3(1), dim3(64), 0, h->stream, h->dev, row, (const double*)accPn_slot(h, t), rec_at(h, t, fused_rec(h)));
  h->pipe.red_pending = true; h->pipe.red_t = t; h->pipe.red_row = row;
}
// ... or at once (init, end of a run), on the MAIN stream: behind the allocation / metrics kernel of the last iteration in
// stream order, and behind the log-prior workgroups of that iteration on the side streams through ONE event wait (they ran
// beside the allocation kernel and are long done).  On the side stream it took two cross-stream hops in a row (side waits
// for main, main waits for side: ~15 us each) at the end of every bnmf_run.
static void flush_reduce(bnmf_handle* h, Timer& tm) {
  if (!h->pipe.red_pending) return;
  if (h->pipe.side_ev_stale) hipEventRecord(h->ev_sideP, h->side2);   // fixed-rank sweep: k_lpp / k_lpe workgroups live on side2
  hipStreamWaitEvent(h->stream, h->ev_sideP, 0);
  issue_pending_reduce(h, tm, h->stream);
}
// P and E updates of the MH models (R/sample_params.R:56-64 with sample_Pn/_En -> *_normal -> MH_*_poisson)
struct MhPipe { MhETail et; MhPTail pt; };
// The instantiation of k_mh_ecol16 (several columns per wave) for a launch: METRICS = the metrics pass (launch_mh_metrics) instead of the
// column sweep; gw = lanes per column (16, else 32); k96 = register arrays for 96 rows instead of MHE16_KMAX.  The Normal forms (fp64 data
// in the registers) and the metrics pass have no MH step.
using MhEcol16 = decltype(&k_mh_ecol16<false, false, 16>);
template <bool METRICS, bool MHSTEP, bool NORMAL>
static MhEcol16 mh_ecol16_shape(int gw, bool k96) {
  if (gw == 16) return k96 ? k_mh_ecol16<METRICS, MHSTEP, 16, 96, NORMAL> : k_mh_ecol16<METRICS, MHSTEP, 16, MHE16_KMAX, NORMAL>;
  return k96 ? k_mh_ecol16<METRICS, MHSTEP, 32, 96, NORMAL> : k_mh_ecol16<METRICS, MHSTEP, 32, MHE16_KMAX, NORMAL>;
}
template <bool METRICS>
static MhEcol16 mh_ecol16_kernel(bool mhstep, int gw, bool k96, bool normal) {
  if (normal) return mh_ecol16_shape<METRICS, false, true>(gw, k96);
  if constexpr (!METRICS) if (mhstep) return mh_ecol16_shape<false, true, false>(gw, k96);
  return mh_ecol16_shape<METRICS, false, false>(gw, k96);
}
static bool mh_ecol16_k96(const bnmf_handle* h) { return h->cfg.K <= 96 && !h->mh.e_k128; }   // BNMF_MHE_K128=1: the 128-row form also where K <= 96
static void launch_mh_PE(bnmf_handle* h, uint32_t t, int converged, bool poll = false, const MhPipe* pp = nullptr) {
  const int K = h->cfg.K, N = h->cfg.N, G = h->cfg.G, S = h->mh.S;
  const bool normal = h->cfg.likelihood == BNMF_NORMAL;
  const int mhstep = (h->cfg.MH && converged && !normal) ? 1 : 0;
  if (pp) {
    if (!h->pipe.mh_pipe_valid) {                                 // first hosted sweep after init / set_array / a sweep of the other form
      hipMemsetAsync(h->mh.dNzE + 2 * N, 0, 4 * N * sizeof(int), h->stream);
      hipLaunchKernelGGL(k_mh_nz, dim3(N), dim3(256), 0, h->stream, h->dev, h->mh.dNzE + 2 * N + ((t - 1) & 1u) * N);
      h->pipe.mh_pipe_valid = true; h->pipe.mh_prep_valid = false;
    }
  } else if (!h->pipe.mh_prep_valid) {                            // first sweep after init / set_array; afterwards k_mh_tail prepares them
    hipMemsetAsync(h->mh.dNzE, 0, 2 * N * sizeof(int), h->stream);         // nzE[N], nzP[N]
    hipLaunchKernelGGL(k_mh_nz, dim3(N), dim3(256), 0, h->stream, h->dev, h->mh.dNzE);
    h->pipe.mh_prep_valid = true; h->pipe.mh_pipe_valid = false;
  }
  assert(!(h->pipe.mh_prep_valid && h->pipe.mh_pipe_valid));
  double* accP = h->arr[BNMF_ACC_P].d; double* accE = h->arr[BNMF_ACC_E].d;
  const bool regP = S <= MHP_W && !h->mh.no_reg;                              // one 320-column segment per wave: the row's cells stay in registers
  const size_t ldsP = (4 * (size_t)S + 2 * N + 2 + (size_t)(PRE_W + 2) * N + ((regP && mhstep) ? (size_t)MH_CPL * MHP_T : 0)) * sizeof(double);
  const bool pipe = pp != nullptr;                         // hosted form (sweep_mh): parity flag buffers, hosted workgroups behind the rows / the column blocks
  int* const nzb = h->mh.dNzE + 2 * N;                        // nzE[2][N], nzP[2][N]
  const int* nzE_in = pipe ? nzb + ((t - 1) & 1u) * N : h->mh.dNzE;
  int* nzP_io = pipe ? nzb + 2 * N + (t & 1u) * N : h->mh.dNzE + N;
  const MhETail et = pipe ? pp->et : MhETail{};
  const int nhostP = pipe ? mh_etail_groups(et, N, MHP_T / ES_T) : 0;
  const size_t ldsPx = pipe ? std::max<size_t>(ldsP, MHP_T * sizeof(double)) : ldsP;
  auto goP = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(K + nhostP), dim3(MHP_T), ldsPx, h->stream, h->dev, t, S, nzE_in, nzP_io, accP, h->mh.dMhat, h->mh.dMhat + (size_t)K * h->cfg.G,
                                                poll ? SideWait{h->dFlags + 1, h->dFlags + 1, t, h->dErr} : SideWait{}, et); };
  if (normal) { if (regP) goP(k_mh_prow<true, true, false>); else goP(k_mh_prow<true, false, false>); }
  else if (mhstep) { if (regP) goP(k_mh_prow<false, true, true>); else goP(k_mh_prow<false, false, true>); }
  else { if (regP) goP(k_mh_prow<false, true, false>); else goP(k_mh_prow<false, false, false>); }
  int grid = (G + 3) / 4; if (grid > 2048) grid = 2048;
  if (h->mh.e16) {                                          // several columns per wave
    // lanes per column: 16 for the Gibbs-only sweep, 32 with the MH step (measured at config 3: 117 / 126 us and 276 / 205 us)
    const int gw = h->mh.e_gw ? h->mh.e_gw : (mhstep ? 32 : 16), cpw = 64 / gw;
    int g16 = ((G + cpw - 1) / cpw + 3) / 4; if (g16 > 2048) g16 = 2048;
    const size_t lds16 = (4 * (size_t)cpw * N * (1 + PRE_W) + 2 * (size_t)N) * sizeof(double);
    const MhPTail pt = pipe ? pp->pt : MhPTail{};
    const int nhostE = pipe ? mh_ptail_blocks(pt, N, h->cfg.MH) : 0;
    const size_t lds16x = pipe ? std::max<size_t>(lds16, RT * sizeof(double)) : lds16;
    int* nzE_set = pipe ? nzb + (t & 1u) * N : nullptr;
    const MhEcol16 kern = mh_ecol16_kernel<false>(mhstep != 0, gw, mh_ecol16_k96(h), normal);
    hipLaunchKernelGGL(kern, dim3(g16 + nhostE), dim3(MHE_T), lds16x, h->stream, h->dev, t, (const int*)nzP_io, accE, 0, nzE_set, g16, pt);
  } else if (normal)
  hipLaunchKernelGGL((k_mh_ecol<false, true>), dim3(grid), dim3(MHE_T), h->mh.e_lds, h->stream, h->dev, t, 0, (const int*)(h->mh.dNzE + N), accE, 0);
  else
  hipLaunchKernelGGL(k_mh_ecol<false>, dim3(grid), dim3(MHE_T), h->mh.e_lds, h->stream, h->dev, t, mhstep, (const int*)(h->mh.dNzE + N), accE, 0);
}
static int launch_mh_metrics(bnmf_handle* h, uint32_t t, bool cells, bool with_record = false, bool with_side = false) {   // with_record: record_sample inside k_mh_tail; with_side: and the hyper sweep of t + 1
  const int draw_sig = h->cfg.likelihood == BNMF_NORMAL ? 1 : 0;
  if (draw_sig) cells = true;                 // sigmasq is drawn after R, A (R/sample_params.R:86-88) in the metrics pass
  const int N = h->cfg.N, G = h->cfg.G;
  if (cells) {
    if (h->mh.e16) {
      const int gw = h->mh.e_gw ? h->mh.e_gw : 16, cpw = 64 / gw;
      int g16 = ((G + cpw - 1) / cpw + 3) / 4; if (g16 > 2048) g16 = 2048;
      const size_t lds16 = (4 * (size_t)cpw * N * (1 + PRE_W) + 2 * (size_t)N) * sizeof(double);
      const MhEcol16 kern = mh_ecol16_kernel<true>(false, gw, mh_ecol16_k96(h), draw_sig != 0);
      hipLaunchKernelGGL(kern, dim3(g16), dim3(MHE_T), lds16, h->stream, h->dev, t, (const int*)nullptr, h->arr[BNMF_ACC_E].d, draw_sig, (int*)nullptr, g16, MhPTail{});
    } else {
      int grid = (G + 3) / 4; if (grid > 2048) grid = 2048;
      if (draw_sig) hipLaunchKernelGGL((k_mh_ecol<true, true>), dim3(grid), dim3(MHE_T), h->mh.e_lds, h->stream, h->dev, t, 0, (const int*)nullptr, h->arr[BNMF_ACC_E].d, draw_sig);
      else hipLaunchKernelGGL(k_mh_ecol<true>, dim3(grid), dim3(MHE_T), h->mh.e_lds, h->stream, h->dev, t, 0, (const int*)nullptr, h->arr[BNMF_ACC_E].d, draw_sig);
    }
  }
  // log-priors and acceptance sums, (for the next iteration's P sweep) Et, nzE, nzP = 0, and record_sample: one launch
  RecArgs ra{};
  if (with_record) { if (int rc = record_args(h, t, ra)) return rc; }
  const int nrec = (ra.n > 0 || ra.Rdst) ? 256 : 0;
  // the canonical reductions of the iteration BEFORE ride in this launch when the hyper sweep runs on the main stream (launch_side_main):
  // as a kernel of their own on the side stream nothing ordered the writers of their slot, three iterations on, behind them
  const RedSlots rs = h->mh.side_main ? take_reduce_slots(h) : RedSlots{};
  SideInTail sx{};
  if (with_side) {                                           // launch_side_main's kernel as the first blocks of this one
    const int nbP = side_nbP(h), nbE = side_nbE(h);
    sx = SideInTail{N + nbP + nbE, nbP, t + 1, rec_at(h, t + 1, fused_rec(h))};
    h->pipe.flags_valid = false; h->pipe.side_valid = true; h->pipe.side_main = true;
  }
  hipLaunchKernelGGL(k_mh_tail, dim3(sx.n + 2 * N + h->nblkE + nrec + (rs.on ? (h->cfg.MH ? 5 : 4) : 0)), dim3(ES_T), 0, h->stream, h->dev, t, (const double*)h->arr[BNMF_ACC_P].d, accPn_slot(h, t),
                     (const double*)h->arr[BNMF_ACC_E].d, accEp_slot(h, t), h->mh.dNzE, h->mh.dNzE + N, h->nblkE, ra, nrec, rs, sx);
  h->pipe.mh_prep_valid = true;
  return 0;
}
// record_sample's arrays of iteration t in two groups: what the row sweep of t + 1 rewrites (P, its prior parameters of t, its acceptance
// rates: copied beside the column sweep of t) and the rest (copied beside the row sweep of t + 1)
static int record_args_split(bnmf_handle* h, uint32_t t, RecArgs& raP, RecArgs& raE) {
  RecArgs ra;
  if (int rc = record_args(h, t, ra)) return rc;
  raP = RecArgs{}; raE = RecArgs{};
  raE.R = ra.R; raE.Rdst = ra.Rdst;
  const int pids[] = {BNMF_P, BNMF_ACC_P, BNMF_MU_P, BNMF_SIGMASQ_P, BNMF_LAMBDA_P, BNMF_ALPHA_P, BNMF_BETA_P};
  for (int j = 0; j < ra.n; ++j) {
    bool isP = false;
    for (int id : pids) { const Arr& a = h->arr[id]; if (a.ring && ra.dst[j] >= a.ring && ra.dst[j] < a.ring + (size_t)h->wcap * id_len(h, id)) isP = true; }
    RecArgs& o = isP ? raP : raE;
    o.src[o.n] = ra.src[j]; o.dst[o.n] = ra.dst[j]; o.len[o.n] = ra.len[j]; o.n++;
  }
  return 0;
}
static MhETail mh_etail_args(bnmf_handle* h, uint32_t te, uint32_t t_next, int& rc) {   // the E side of iteration te (0: none pending); t_next: the iteration of the next column sweep
  const int N = h->cfg.N;
  MhETail et{};
  rc = 0;
  et.nz_zero = h->mh.dNzE + 2 * N + (t_next & 1u) * N;
  if (!te) return et;
  RecArgs raP;
  if ((rc = record_args_split(h, te, raP, et.ra))) return et;
  et.on = 1; et.t = te;
  et.nbE = side_nbE(h); et.nblkE = h->nblkE;
  et.nrec = (et.ra.n > 0 || et.ra.Rdst) ? 128 : 0;
  et.accE = h->arr[BNMF_ACC_E].d; et.accE_part = accEp_slot(h, te); et.lpE_part = h->dlpE + (size_t)(te % 3u) * h->nblkE;
  return et;
}
// the E side of the last iteration of a call: no row sweep behind it
static int flush_mh_etail(bnmf_handle* h) {
  if (!h->pipe.mh_etail_pending) return 0;
  int rc = 0;
  const MhETail et = mh_etail_args(h, h->pipe.mh_etail_pending, h->pipe.mh_etail_pending + 1, rc);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mh_etail, dim3(mh_etail_groups(et, h->cfg.N, 4)), dim3(1024), 0, h->stream, h->dev, et);
  h->pipe.mh_etail_pending = 0;
  return 0;
}
// The hosted form of the sweep (Poisson MH models at fixed rank, k_mh_ecol16): two launches per iteration, k_mh_tail's work inside them (mh.h)
static int sweep_mh_pipe(bnmf_handle* h, int row, int converged, Timer& tm) {
  h->iter += 1;
  const uint32_t t = (uint32_t)h->iter;
  const int N = h->cfg.N;
  use_slot(h, t);
  if (!h->pipe.side_valid) launch_side(h, t, tm);              // first sweep after init / set_array: the prior parameters of t on the side streams
  assert(h->pipe.side_valid && !(h->pipe.side_main && h->pipe.flags_valid));
  if (!h->pipe.side_main) { refresh_side_events(h); hipStreamWaitEvent(h->stream, h->ev_side, 0); hipStreamWaitEvent(h->stream, h->ev_sideP, 0); }
  MhPipe pp{};
  int rc = 0;
  pp.et = mh_etail_args(h, h->pipe.mh_etail_pending, t, rc);
  if (rc) return rc;
  MhPTail& pt = pp.pt;
  pt.on = 1; pt.t = t;
  pt.nbP = side_nbP(h);
  RecArgs raE;
  if ((rc = record_args_split(h, t, pt.ra, raE))) return rc;
  pt.nrec = pt.ra.n > 0 ? 8 : 0;
  pt.accP = h->arr[BNMF_ACC_P].d; pt.accPn = accPn_slot(h, t);
  pt.nblkE = h->nblkE;
  pt.nz_zero = h->mh.dNzE + 2 * N + 2 * N + ((t + 1) & 1u) * N;
  pt.rs = take_reduce_slots(h);                            // k_reduce's work for the iteration before: its E-side sums are issued with pp.et above
  dbg_delay_main(h);
  launch_mh_PE(h, t, converged, false, &pp);
  dbg_delay_main(h);
  h->pipe.mh_etail_pending = t;
  h->pipe.flags_valid = false; h->pipe.side_valid = true; h->pipe.side_main = true;
  launch_reduce(h, t, row, tm);
  return 0;
}
static int sweep_mh(bnmf_handle* h, int row, int converged, Timer& tm) {
  if (h->mh.pipe && !tm.on) return sweep_mh_pipe(h, row, converged, tm);
  if (int rc = flush_mh_etail(h)) return rc;
  h->iter += 1;
  const uint32_t t = (uint32_t)h->iter;
  use_slot(h, t);
  if (!h->pipe.side_valid) launch_side(h, t, tm);
  assert(h->pipe.side_valid && !(h->pipe.side_main && h->pipe.flags_valid));
  // prior parameters of iteration t: in the steady state the P-row kernel polls the flag k_side publishes (a stream wait is a
  // barrier packet: ~16 us of bubble per iteration here); after init / set_array / in profile mode a stream wait
  const bool on_main = h->pipe.side_main;                       // the hyper sweep of t ran on this stream (launch_side_main): nothing to wait for
  const bool poll = !on_main && h->pipe.flags_valid && !tm.on && !h->serial;
  if (!poll && !on_main) { refresh_side_events(h); hipStreamWaitEvent(h->stream, h->ev_side, 0); hipStreamWaitEvent(h->stream, h->ev_sideP, 0); }
  dbg_delay_main(h);
  tm.begin(KN_MH, h->stream); launch_mh_PE(h, t, converged, poll); tm.end(KN_MH, h->stream);
  dbg_delay_main(h);
  // the hyper sweep of t + 1: on the main stream — inside k_mh_tail below (its own launch in profile mode, which times it) — or on the side stream
  const bool side_in_tail = h->mh.side_main && !tm.on && h->mh.side_tail;
  if (side_in_tail) {} else if (h->mh.side_main) launch_side_main(h, t + 1, tm); else launch_side(h, t + 1, tm, !tm.on);
  if (h->cfg.learning_rank) { tm.begin(KN_RANK, h->stream); launch_rank(h, t); tm.end(KN_RANK, h->stream); }
  // record_sample rides in k_mh_tail: after sample_sigmasq, like record_sample (:279) after sample_params (:276)
  tm.begin(KN_OTHER, h->stream); if (int rc = launch_mh_metrics(h, t, h->cfg.learning_rank != 0, true, side_in_tail)) return rc; tm.end(KN_OTHER, h->stream);
  launch_reduce(h, t, row, tm);
  return 0;
}
// Merged draw kernel + gate at the end of the allocation kernel (k_draw, zalloc_reg.h): pays when the allocation kernel is long
// enough to cover the side streams' kernels that its last lane waits for: 107 -> 92.5 us per iteration at K = 96, G = 10,000, 59.4 -> 52.7 at
// G = 3,000, but 45.2 -> 51.1 us at G = 2,000, where they outlast the kernel and the gate puts them on the main stream's path.
// BNMF_GATE=0 / 1 forces it off / on (diagnostics).
static bool gate_enabled(const bnmf_handle* h) {
  if (h->gate_forced >= 0) return h->gate_forced != 0;
  // tools/gatesize.py (us per iteration without / with, K = 96, N = 20, recording on).  Round 3: 45.2 / 51.1 at G = 2,000; 59.4 / 52.7 at G = 3,000;
  // 107 / 92.5 at G = 10,000 -> from 250,000 cells.  Round 5 (the sorted schedule without metric tasks, the two draw kernels' and the side
  // kernels' chains shortened): 48.3 / 55.4 at G = 3,000; 56.4 / 58.9 at 4,000; 63.6 / 59.3 at 5,000; 72.4 / 67.0 at 7,000; 85.9 / 84.1 at
  // 10,000 -> the crossover has moved up; with the quads per item chosen per data set (build_zsort): 45.5 / 52.9 at G = 3,000; 49.0 / 54.3 at 4,000;
  // 59.8 / 60.6 at 5,000; 72.7 / 68.9 at 7,000; 85.6 / 83.5 at 10,000
  return (size_t)h->cfg.K * h->cfg.G >= 550000;
}
// ... and what the handle's configuration must allow beside it: fixed rank, the register allocation kernel or a schedule on top of it
static bool merged_draw_ok(const bnmf_handle* h) { return gate_enabled(h) && !h->cfg.learning_rank && (h->zkind == ZKind::reg || h->zkind == ZKind::sort); }
// workgroup width of the merged draw kernel: the E elements spread over (almost) all CUs in ONE round of workgroups — 1,024-lane workgroups
// left 60 of 256 CUs idle at N G = 200,000 — while the workgroup count stays small (the gap to the next kernel grows with it)
static int ensure_draw_bw(bnmf_handle* h) {
  if (h->draw_bw) return 0;
  hipDeviceProp_t pr;
  HIPCHK(hipGetDeviceProperties(&pr, h->device));
  const size_t per_cu = ((size_t)h->cfg.N * h->cfg.G + pr.multiProcessorCount - 1) / pr.multiProcessorCount;
  size_t bw = ((per_cu + 63) / 64) * 64 + 64;        // one wave of slack: a few CUs take two small workgroups rather than one a second round
  h->draw_bw = (int)std::min<size_t>(DW, std::max<size_t>(256, bw));
  if (const char* e = getenv("BNMF_DRAWBW")) { const int v = atoi(e); if (v >= 64 && v <= DW && v % 64 == 0) h->draw_bw = v; }   // diagnostics
  return 0;
}
// May this launch take the geometry-fixed form of k_draw (kernels.h DrawFixed)?  Everything FX turns into a constant is checked against what the
// dynamic form would read from the same arguments: K, N, the width, the Gamma prior, every ring pointer of the fused recording, no
// accumulating ZsumK, no fixed column; and the element index must fit the form's 32 bits.  BNMF_DRAWFIXED=0 (read at bnmf_create): never.
template <class FX>
static bool draw_fixed_form(const bnmf_handle* h, const RecDst& r, const RecDst& rn) {
  const Dev& d = h->dev;
  const bool rec_set = r.P && r.E && r.A && r.R && rn.pp[2] && rn.pp[3];
  return h->draw_fixed_ok && d.K == FX::K && d.N == FX::N && h->draw_bw == FX::BW && d.prior == BNMF_GAMMA && !h->cfg.learning_rank &&
         rec_set == FX::rec && (FX::rec || !(r.P || r.E || r.A || r.R || rn.pp[2] || rn.pp[3])) && !d.zsumk_accum && !d.fixedP &&
         d.lenE <= (size_t)INT32_MAX - DW;
}
// The head of the two-kernel sweeps (fixed rank and rank learning): k_pdraw, its completion as a stop event (ev_p: no marker packet on the
// main stream)
static void launch_pdraw_split(bnmf_handle* h, uint32_t t, bool rec, bool poll) {
  // The side work of this iteration may have been issued by launch_side_merged (the sweep before took the merged path without
  // arming the allocation kernel's gate: first sweep after init / set_array).  Its P-side sweep then runs on `side` under flag
  // [9], which k_pdraw does not poll ([1] was raised by k_draw, [3] covers side2 only): the main stream waits for it here, and
  // with it launch_side_P (released by k_pdraw's stop event) cannot overwrite the slot that sweep still reads.
  if (poll && h->pipe.gate_f0 == 9) { hipEventRecord(h->ev_side, h->side); hipStreamWaitEvent(h->stream, h->ev_side, 0); }
  if (h->cfg.learning_rank) flush_colterms(h);           // (fixed rank: launch_side_E takes the column terms of t - 1 along)
  hipExtLaunchKernelGGL(k_pdraw, dim3(h->cfg.N), dim3(PD_T), (uint32_t)(2 * (size_t)h->cfg.K * sizeof(double)), h->stream,
                        nullptr, h->ev_p, 0, h->dev, t, 0, 0, rec_pdraw(h, t, rec),
                        poll ? SideWait{h->dFlags + 1, h->dFlags + 3, t, h->dErr} : SideWait{}, (const int*)nullptr);
  h->pipe.gate_f0 = 1;
}
static void launch_edraw_split(bnmf_handle* h, uint32_t t, bool rec) {   // ... and k_edraw, its completion as ev_draw
  hipExtLaunchKernelGGL(k_edraw, dim3(h->nblkE), dim3(ES_T), 0, h->stream, nullptr, h->ev_draw, 0, h->dev, t, 0, 0, rec_at(h, t, rec).E);
}
static int sweep(bnmf_handle* h, int row, Timer& tm) {
  h->iter += 1;
  const uint32_t t = (uint32_t)h->iter;
  use_slot(h, t);
  const bool rec = fused_rec(h);
  if (!h->pipe.side_valid) launch_side(h, t, tm);               // first sweep after init / set_array
  assert(h->pipe.side_valid && !h->pipe.side_main);        // the Gibbs sweep never runs its hyper sweep on the main stream
  // The log-prior kernel of iteration t-1 (k_lpe, side stream) is ordered only behind its own inputs, not before this
  // iteration's k_edraw.  With recording on it reads E_{t-1} from the ring; without a ring E is double-buffered: this k_edraw
  // writes the buffer that held E_{t-2}.  Nothing below reads E_{t-1}: the draws use ZsumK / Psum / Esum, everything after
  // k_edraw works on E_t.  (The P side needs nothing: k_lpp precedes Esum, whose flag releases k_pdraw.)
  if (!lpe_from_ring(h)) {
    if (!h->E_alt) {
      HIPCHK(dmalloc(&h->E_alt, (size_t)h->cfg.N * h->cfg.G * sizeof(double)));
      HIPCHK(hipMemsetAsync(h->E_alt, 0, (size_t)h->cfg.N * h->cfg.G * sizeof(double), h->stream));
    }
    std::swap(h->arr[BNMF_E].d, h->E_alt);
    h->dev.E = h->arr[BNMF_E].d;
  }
  // THE CHOICE.  poll: the prior parameters + Esum of iteration t reach the draws through the flags their kernels publish (steady state:
  // no barrier packet on the main stream); else through a stream wait (after init / set_array, in profile mode, serial mode).
  // The merged draw kernel needs the allocation kernel of t-1 to have waited for this iteration's hyper sweep (its gate), or the main
  // stream to have (the event wait below); the allocation kernel of t is gated in its turn whenever the next sweep could poll.
  enum Body { PROFILE, MERGED, SPLIT, RANK };
  const bool poll = h->pipe.flags_valid && !tm.on && !h->serial;
  const bool merged_ok = merged_draw_ok(h);
  const Body body = tm.on ? PROFILE : (merged_ok && (!poll || h->pipe.z_gated_for == t)) ? MERGED : h->cfg.learning_rank ? RANK : SPLIT;
  const bool gate = merged_ok && poll;
  assert(h->pipe.gate_f0 == 1 || (h->pipe.gate_f0 == 9 && !h->cfg.learning_rank));   // only launch_side_merged leaves 9
  assert(h->pipe.z_gated_for != t || merged_ok);           // only a gated allocation kernel leaves z_gated_for = t

  if (!poll) { refresh_side_events(h); hipStreamWaitEvent(h->stream, h->ev_side, 0); }
  dbg_delay_main(h);
  switch (body) {
    case PROFILE:                                            // one kernel at a time
      flush_colterms(h);
      tm.begin(KN_PDRAW, h->stream); launch_pdraw(h, t, 0, rec); tm.end(KN_PDRAW, h->stream);
      tm.begin(KN_EDRAW, h->stream); launch_edraw(h, t, 0, rec); tm.end(KN_EDRAW, h->stream);
      launch_side(h, t + 1, tm);
      if (h->cfg.learning_rank) { tm.begin(KN_RANK, h->stream); launch_rank(h, t, nullptr, row); tm.end(KN_RANK, h->stream); }
      break;
    case MERGED: {                                           // k_draw (P, E and the E-side hyper sweep of t + 1), its completion as ev_draw
      if (int rc = ensure_draw_bw(h)) return rc;
      const unsigned bw = (unsigned)h->draw_bw;
      const unsigned nE = (unsigned)(((size_t)h->cfg.N * h->cfg.G + bw - 1) / bw);
      const RecDst r = rec_at(h, t, rec), rn = rec_at(h, t + 1, rec);
      auto go = [&](auto kernel) {
        hipExtLaunchKernelGGL(kernel, dim3(h->cfg.N + nE), dim3(bw), 0, h->stream, nullptr, h->ev_draw, 0, h->dev, t, r,
                              SideDone{h->dFlags + 5, h->dFlags + 6, (unsigned)h->cfg.N, t}, SideWait{h->dFlags + 6, h->dFlags + 6, t, h->dErr},
                              rn, SideDone{h->dFlags, h->dFlags + 1, nE, t + 1}, h->dDrawOwn, ++h->draw_seq, h->dbg_draw_no_p);
      };
      if (draw_fixed_form<DrawFixHead>(h, r, rn)) {          // the metric configuration with recording on: K, N, the width, the prior and the ring pointers as constants
        assert((size_t)h->cfg.N * h->cfg.G == h->dev.lenE && h->dev.lenE + DW <= (size_t)INT32_MAX);   // its element index has 32 bits
        go(k_draw_fixed<DrawFixHead>);
      } else go(k_draw);
      launch_side_merged(h, t + 1, tm);
      break;
    }
    case SPLIT:                                              // fixed rank, two draw kernels
      launch_pdraw_split(h, t, rec, poll);
      launch_side_P(h, t + 1);
      launch_edraw_split(h, t, rec);
      launch_side_E(h, t + 1, tm);                           // overlaps k_zalloc below
      break;
    case RANK:
      // every workgroup of the rank sweep waits for all others at every factor, so a kernel sharing a CU with one of them delays
      // the whole grid: see launch_side_early / launch_side_late
      launch_pdraw_split(h, t, rec, poll);
      launch_edraw_split(h, t, rec);
      launch_side_early(h, t + 1);
      launch_rank(h, t, h->ev_rank, row);
      launch_side_late(h, t + 1, tm);
      break;
  }
  h->pipe.z_gate_next = gate ? t + 1 : 0u;
  dbg_delay_main(h);
  tm.begin(KN_ZALLOC, h->stream);
  if (int rc = launch_zalloc(h, t)) return rc;
  tm.end(KN_ZALLOC, h->stream);
  if (h->zkind == ZKind::sort) {
    h->pipe.ct_pending = t;
    if (tm.on) { tm.begin(KN_OTHER, h->stream); flush_colterms(h); tm.end(KN_OTHER, h->stream); }   // profile mode: the column terms as a launch of their own ("other")
  }
  h->pipe.z_gated_for = h->pipe.z_gate_next; h->pipe.z_gate_next = 0;
  record_Z(h, t);
  launch_reduce(h, t, row, tm, h->cfg.learning_rank != 0);
  return 0;
}

// Two handles that learn the rank must not run on one device at the same time: each persistent rank sweep sizes its grid
// as if it owned the device (one workgroup per CU, every workgroup waits for all others), and two half-resident grids
// would wait for each other until their bounded spins give up.  Their calls take turns (a call is at most one block of
// iterations between MAP checks).  Nor may a rank-learning call run beside ANY other chain's call on the device (round 4, found
// by tools/concurrent_check.py with full-size chains): a workgroup that waits inside a kernel for its chain's side streams (the
// allocation kernel's gate, the draw kernels' polls) holds a CU the rank sweep's grid needs, while the rank sweep's resident
// workgroups hold the registers the side-stream kernel needs — a cycle only the time-outs broke.  Rank-learning calls take the
// device's lock exclusively, all other calls shared.
static int flock_retry(int fd, int op) { int rc; while ((rc = flock(fd, op)) != 0 && errno == EINTR) {} return rc; }
static int run_impl(bnmf_handle* h, int n_iter, int converged, double* metrics, Timer& tm) {
  if (!h) return fail(BNMF_EINVAL, "bnmf_run: null handle");
  const bool excl = h->cfg.learning_rank != 0;
  // The rule between the PROCESSES that share the device first (each learns nothing of the others' launches), then the one between the
  // chains of this process — a call blocked on another process must not hold this process's gate.  Without the lock files a
  // rank-learning call is refused (two such chains of two processes end in each other's time-outs) unless the caller has said
  // BNMF_DEVLOCK=0: no other process uses the device.
  struct FileTurn { int fd; ~FileTurn() { if (fd >= 0) flock(fd, LOCK_UN); } } fturn{-1};
  if (!h->devlock_off) {
    if (h->devlock_fd < 0 || h->devgate_fd < 0) {
      if (excl) return fail(BNMF_ESTATE, "bnmf_run: a rank-learning chain needs its device to itself, and the device's lock files could not be opened "
                                         "(see the warning at bnmf_create): set BNMF_LOCKDIR, or BNMF_DEVLOCK=0 if no other process uses this GPU");
    } else {
      int rc;
      if (excl) { rc = flock_retry(h->devgate_fd, LOCK_EX); if (!rc) { rc = flock_retry(h->devlock_fd, LOCK_EX); flock(h->devgate_fd, LOCK_UN); } }
      else { rc = flock_retry(h->devgate_fd, LOCK_SH); if (!rc) { flock(h->devgate_fd, LOCK_UN); rc = flock_retry(h->devlock_fd, LOCK_SH); } }
      if (rc) return fail(BNMF_ESTATE, "bnmf_run: the device's lock file could not be taken (%s)", strerror(errno));
      fturn.fd = h->devlock_fd;
    }
  }
  struct GateTurn { DeviceGate* g; bool ex; ~GateTurn() { if (g) { if (ex) g->unlock(); else g->unlock_shared(); } } } gturn{nullptr, excl};
  if (h->device >= 0 && h->device < 64) {
    gturn.g = &g_dev_gate[h->device];
    if (excl) gturn.g->lock(); else gturn.g->lock_shared();
  }
  if (!h->inited) return fail(BNMF_ESTATE, "bnmf_run: call bnmf_init first");
  if (h->poisoned) return fail(BNMF_ESTATE, "bnmf_run: an earlier call timed out inside a kernel; the handle's state is invalid, destroy it");
  if (n_iter < 0) return fail(BNMF_EINVAL, "bnmf_run: n_iter < 0");
  if (n_iter == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ensure_metrics(h, (size_t)n_iter)) return rc;
  const uint32_t t0 = (uint32_t)h->iter + 1;
  // BNMF_RUNCLOCK=1 (diagnostics): host time of the call's phases on stderr
  static const bool runclock = getenv("BNMF_RUNCLOCK") != nullptr;
  const auto rc0 = std::chrono::steady_clock::now();
  auto rc_us = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - rc0).count(); };
  double rc_first = 0.0, rc_issued = 0.0, rc_tail = 0.0, rc_main = 0.0;
  for (int i = 0; i < n_iter; ++i) {
    if (runclock && i == 1) rc_first = rc_us();
    if (int rc = ((h->cfg.MH || h->cfg.likelihood == BNMF_NORMAL) ? sweep_mh(h, i, h->cfg.MH ? converged : 0, tm) : sweep(h, i, tm))) return rc;
    HIPCHK(hipGetLastError());                               // a refused launch of this iteration (bad geometry, LDS size)
    // a bounded in-kernel wait that timed out has set its word (mapped host memory): issue nothing more, so that one stuck
    // hand-off costs one spin bound and not one per remaining launch
    if (((volatile int*)h->hErr)[0] | ((volatile int*)h->hErr)[1]) break;
  }
  if (runclock) rc_issued = rc_us();
  flush_colterms(h);                                       // the last iteration's column terms: no draw kernel behind it in this call
  if (int rc = flush_mh_etail(h)) return rc;              // (hosted MH sweep) the last iteration's E side: no row sweep behind it in this call
  // Round 5: the main stream waits for EVERYTHING issued on the two side streams (a fresh event each) in front of the last reduction:
  // when it is idle so are they, and the two host-side synchronisations of idle streams that stood below (6 us each, at the end of
  // every call) are gone.  (flush_reduce's own wait for side2 is then a wait for an event that has fired.)
  hipEventRecord(h->ev_z, h->side); hipStreamWaitEvent(h->stream, h->ev_z, 0);
  hipEventRecord(h->ev_sideP, h->side2); hipStreamWaitEvent(h->stream, h->ev_sideP, 0);
  if (h->pipe.side_ev_stale) chain_ev_side(h);            // refresh_side_events, whose ev_sideP is the one just recorded (the main stream's wait stays in between)
  flush_reduce(h, tm);
  hipLaunchKernelGGL(k_compose, dim3((n_iter + 63) / 64), dim3(64), 0, h->stream, h->dev, n_iter, t0);
  HIPCHK(hipGetLastError());
  std::vector<double> own;
  if (!metrics && h->wcap > 0) { own.resize((size_t)n_iter * BNMF_NMETRIC); metrics = own.data(); }
  if (runclock) rc_tail = rc_us();
  HIPCHK(hipStreamSynchronize(h->stream));
  if (runclock) rc_main = rc_us();
  if (metrics) memcpy(metrics, h->hMetrics, (size_t)n_iter * BNMF_NMETRIC * sizeof(double));

  if (runclock) fprintf(stderr, "[bnmf_run %d] first iteration issued %.1f us, all issued %.1f, tail issued %.1f, main stream idle %.1f, side streams idle %.1f\n",
                        n_iter, rc_first, rc_issued, rc_tail, rc_main, rc_us());
  if (h->wcap > 0 && metrics) {                             // loglik / logpost of the recorded iterations (MAP metrics are window means)
    if (h->hist.size() != (size_t)h->wcap * 4) h->hist.assign((size_t)h->wcap * 4, std::nan(""));
    for (int i = 0; i < n_iter; ++i) {
      const double* r = metrics + (size_t)i * BNMF_NMETRIC;
      double* d = h->hist.data() + (size_t)((t0 + i - 1) % (uint32_t)h->wcap) * 4;
      d[0] = r[3]; d[1] = r[4]; d[2] = r[9]; d[3] = r[10];
    }
  }
  // all three streams are idle: the time-out words (mapped host memory) are final
  if (((volatile int*)h->hErr)[0] | ((volatile int*)h->hErr)[1]) {
    // the kernels behind the time-out ran on inputs that were never published: P, E, the rings and the metric rows of this call
    // are not the chain's.  The handle stays poisoned (every later call fails with BNMF_ESTATE) until it is destroyed.
    h->poisoned = true;
    unsigned fl[16] = {};
    hipMemcpy(fl, h->dFlags, sizeof fl, hipMemcpyDeviceToHost);
    if (((volatile int*)h->hErr)[0])
      return fail(BNMF_EHIP, "bnmf_run: a kernel timed out waiting for the hyper-parameter sweep of its iteration (iteration %d; flags E-side %u, Esum %u, P-side %u, draw %u; "
                  "serialised dispatch? set BNMF_SERIAL=1); the handle is now invalid", h->iter, fl[1], fl[3], fl[9], fl[6]);
    return fail(BNMF_EHIP, "bnmf_run: the grid barrier of the rank sweep timed out at iteration %d (workgroups not co-resident?); the handle is now invalid", h->iter);
  }
  return 0;
}
