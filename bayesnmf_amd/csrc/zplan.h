// bayesnmf_amd/csrc/zplan.h — everything bnmf_create decides by arithmetic, as pure host code: no HIP call, no handle.
// The environment switches (Switches), the geometry of the wave-per-column and tile allocation kernels (plan_zwave, plan_ztile), the
// rank sweep's variant and grid (plan_rank), the MH / Normal sweeps' kernels (plan_mh), and the static schedules of k_zalloc_sort and
// k_zalloc_step (plan_zsort, plan_zstep).  Included by api.hip (one translation unit): create_impl there calls the planners and
// allocates / uploads what they return; bnmf_test_zsort_plan / bnmf_test_zstep_plan hand the two schedules to
// tests/test_schedule_host.py on any machine.  A planner that refuses a shape says so with fail() and returns its code.

// ---- the environment switches of a handle (diagnostics / tests; the table is in tools/README.md) ----
// Read at EVERY bnmf_create (tests set them per handle in one process), each in exactly one place: Switches::from_env.  The planners
// take them as values, so a caller decides whether the process environment has a say.
static const int ENV_UNSET = INT_MIN;
static bool env_set(const char* name) { return getenv(name) != nullptr; }
static int env_int(const char* name, int unset = ENV_UNSET, int lo = INT_MIN, int hi = INT_MAX) {
  const char* e = getenv(name);
  return e ? std::max(lo, std::min(hi, atoi(e))) : unset;
}
static bool env_flag(const char* name, bool unset) { const char* e = getenv(name); return e ? atoi(e) != 0 : unset; }
static double env_real(const char* name, double unset) { const char* e = getenv(name); return e ? atof(e) : unset; }
struct Switches {
  // the handle itself (create_impl)
  bool devlock = true;                 // BNMF_DEVLOCK=0: no lock files
  int gate = -1, serial = -1;          // BNMF_GATE, BNMF_SERIAL: -1 unset, else 0 / 1
  bool mh_side_main = true, mh_side_tail = true;   // BNMF_MHSIDE, BNMF_MHSIDETAIL
  bool draw_no_p = false;              // BNMF_DEBUG_DRAW_NO_P
  bool draw_fixed = true;              // BNMF_DRAWFIXED=0: never the geometry-fixed form of k_draw (sweep.h draw_fixed_form)
  int main_delay_us = 0, allside_delay_us = 0, side_delay_us = 0;   // BNMF_DEBUG_{MAIN,ALLSIDE,SIDE}_DELAY_US, 0..20000
  bool rank_dbg = false, zt_dbg = false;   // BNMF_RANKDBG, BNMF_ZTDBG (set = on): the diagnostic buffers
  bool z_eager = false;                // BNMF_ZEAGER
  int ablate = 0;                      // BNMF_ABLATE (-DBNMF_DIAG builds only)
  // plan_rank
  bool rank_half = true; long rank_grid = 0;   // BNMF_RANKHALF=0: whole blocks; BNMF_RANKGRID: workgroups (0 = unset)
  // plan_mh
  bool mhe_k128 = false, mh_pipe = true; int mhe_gw = 0;   // BNMF_MHE_K128, BNMF_MHPIPE, BNMF_MHE_GW (16 / 32, else by mode)
  // plan_zwave, plan_ztile
  bool z_reg = true, z_chunk = false, z_tile = true, z_nolean = false;   // BNMF_ZREG, BNMF_ZCHUNK, BNMF_ZTILE, BNMF_ZNOLEAN (set = on)
  int zw = ENV_UNSET, z_grid = ENV_UNSET;   // BNMF_ZW, BNMF_ZGRID
  // plan_zsort
  bool zsort = true, zs_spread = true, zs_it16 = true, zs_pk = true;   // BNMF_ZSORT, BNMF_ZSSPREAD, BNMF_ZSIT16, BNMF_ZSPK
  bool zs_fixed = true;                // BNMF_ZSFIXED=0: never a geometry-fixed instantiation of k_zalloc_sort (build_zsort; the planner does not read it)
  int zs_lds_kb = ENV_UNSET, zs_w = ENV_UNSET, zs_qmax = 0;             // BNMF_ZSLDS, BNMF_ZSW, BNMF_ZSQMAX
  // plan_zstep
  bool zstep = true, zp_it16 = true; int zp_gb = 0;   // BNMF_ZSTEP, BNMF_ZPIT16, BNMF_ZPGB
  static Switches from_env() {
    Switches s;
    s.devlock = env_flag("BNMF_DEVLOCK", true);
    s.gate = env_set("BNMF_GATE") ? (int)env_flag("BNMF_GATE", false) : -1;
    s.serial = env_set("BNMF_SERIAL") ? (int)env_flag("BNMF_SERIAL", false) : -1;
    s.mh_side_main = env_flag("BNMF_MHSIDE", true); s.mh_side_tail = env_flag("BNMF_MHSIDETAIL", true);
    s.draw_no_p = env_flag("BNMF_DEBUG_DRAW_NO_P", false); s.draw_fixed = env_flag("BNMF_DRAWFIXED", true);
    s.main_delay_us = env_int("BNMF_DEBUG_MAIN_DELAY_US", 0, 0, 20000);
    s.allside_delay_us = env_int("BNMF_DEBUG_ALLSIDE_DELAY_US", 0, 0, 20000);
    s.side_delay_us = env_int("BNMF_DEBUG_SIDE_DELAY_US", 0, 0, 20000);
    s.rank_dbg = env_set("BNMF_RANKDBG"); s.zt_dbg = env_set("BNMF_ZTDBG");
    s.z_eager = env_flag("BNMF_ZEAGER", false);
#ifdef BNMF_DIAG   /* the builder's diagnostic builds only (tools/bin/, never libbnmf.so): phases of the allocation kernels switched off */
    s.ablate = env_int("BNMF_ABLATE", 0);
#endif
    s.rank_half = env_flag("BNMF_RANKHALF", true);
    if (const char* e = getenv("BNMF_RANKGRID")) s.rank_grid = atol(e);
    s.mhe_k128 = env_flag("BNMF_MHE_K128", false); s.mh_pipe = env_flag("BNMF_MHPIPE", true);
    { const int v = env_int("BNMF_MHE_GW", 0); s.mhe_gw = v == 32 ? 32 : v == 16 ? 16 : 0; }
    s.z_reg = env_flag("BNMF_ZREG", true); s.z_chunk = env_flag("BNMF_ZCHUNK", false);
    s.z_tile = env_flag("BNMF_ZTILE", true); s.z_nolean = env_set("BNMF_ZNOLEAN");
    s.zw = env_int("BNMF_ZW"); s.z_grid = env_int("BNMF_ZGRID");
    s.zsort = env_flag("BNMF_ZSORT", true); s.zs_spread = env_flag("BNMF_ZSSPREAD", true);
    s.zs_it16 = env_flag("BNMF_ZSIT16", true); s.zs_pk = env_flag("BNMF_ZSPK", true); s.zs_fixed = env_flag("BNMF_ZSFIXED", true);
    s.zs_lds_kb = env_int("BNMF_ZSLDS"); s.zs_w = env_int("BNMF_ZSW"); s.zs_qmax = env_int("BNMF_ZSQMAX", 0);
    s.zstep = env_flag("BNMF_ZSTEP", true); s.zp_it16 = env_flag("BNMF_ZPIT16", true); s.zp_gb = env_int("BNMF_ZPGB", 0);
    return s;
  }
};

// ---- the rank sweep (rank.h): variant and grid ----
// Every workgroup of the persistent sweep waits for all others: the grid must be co-resident.  occ_reg / occ_gen: how many workgroups
// of the register / general variant the runtime says fit a CU (registers, LDS); where the answer is SGPR-limited (>= 6 per CU) the
// query can be one high (MI355X_MICROARCH.md), so one is kept in reserve there; never more than one per CU is planned: even compute
// times, and co-resident with margin.  Should the grid still not be co-resident, the bounded spins time out and bnmf_run reports it.
struct RankPlan { bool reg = false, half = false; int grid = 0; };
static RankPlan plan_rank(size_t K, size_t G, int n_cu, int occ_reg, int occ_gen, const Switches& sw) {
  RankPlan p;
  const long NB = ((long)G + RK_MAXC - 1) / RK_MAXC;                 // blocks of 8 columns, one compute wave each
  const long wg_needed = (NB + RK_CW - 1) / RK_CW;                   // RK_CW compute waves + the decision wave per workgroup
  auto cap = [&](int occ) { return (long)std::min(1, occ >= 6 ? occ - 1 : occ) * n_cu; };
  const long cap_reg = cap(occ_reg), cap_gen = cap(occ_gen);
  p.reg = K <= 96 && wg_needed <= cap_reg;               // register variant: rows 64..95 of two columns share a register (rank.h)
  // ... with HALF a block per compute wave where the grid of ten-half-block workgroups is co-resident too (704 lanes, one per CU)
  const long wg_half = (NB + RK_CWH / 2 - 1) / (RK_CWH / 2);
  p.half = p.reg && wg_half <= (long)n_cu && NB <= 1536 && sw.rank_half;   // (1,536: one round of its decision wave's gather, rank.h)
  // (a wider grid with the blocks dealt wave-major over all CUs was measured: no gain, the sweep is bound by the
  // per-factor exchange, not by VALU contention)
  const long cap_used = p.reg ? cap_reg : cap_gen;
  p.grid = p.half ? (int)wg_half : (int)std::min<long>(wg_needed, cap_used);
  if (!p.half && sw.rank_grid >= wg_needed && sw.rank_grid <= cap_used) p.grid = (int)sw.rank_grid;   // diagnostics only
  return p;
}

// ---- the MH / Normal sweeps (mh.h): which column kernel, and what it hosts ----
struct MhPlan {
  int S = 1;                           // segments of a row of the P sweep
  size_t e_lds = 0;                    // k_mh_ecol: per wave E column, A, Mhat column, log(Mhat) and candidates
  bool e16 = false;                    // the column sweep by k_mh_ecol16 (K <= 128 and its LDS fits)
  bool e_raise = false, e16_raise = false;   // k_mh_ecol / k_mh_ecol16 need more than 64 KiB of dynamic LDS: raise their limit
  bool pipe = false;                   // Poisson MH models at fixed rank through k_mh_ecol16: what followed the two sweeps is hosted BY them (BNMF_MHPIPE=0: k_mh_tail)
};
static int plan_mh(size_t K, size_t G, size_t N, bool poisson_mh_fixed_rank, bool side_main, bool side_tail, const Switches& sw, MhPlan& p) {
  p = MhPlan();
  p.S = (int)((G + MH_SEG - 1) / MH_SEG);
  p.e_lds = 4 * (2 * N + 3 * K) * sizeof(double);
  if (p.e_lds > 160 * 1024) return fail(BNMF_EINVAL, "bnmf_create: K = %zu too large for the column kernel of the MH / Normal models (LDS)", K);
  p.e_raise = p.e_lds > 64 * 1024;
  // k_mh_ecol16 (K <= 128: several columns per wave): its LDS grows with N — above 64 KiB it needs the attribute, above the CU's 160 KiB
  // the sweep takes k_mh_ecol
  const size_t lds16_max = (4 * (size_t)4 * N * (1 + PRE_W) + 2 * N) * sizeof(double);   // 16 lanes per column: 4 columns per wave
  p.e16 = K <= (size_t)MHE16_KMAX && lds16_max <= 160 * 1024;
  p.e16_raise = p.e16 && lds16_max > 64 * 1024;
  // k_mh_tail's work hosted by the two sweep kernels (mh.h) — the Poisson MH models at fixed rank where the column sweep is k_mh_ecol16
  p.pipe = p.e16 && poisson_mh_fixed_rank && side_main && side_tail && N <= RT && sw.mh_pipe;
  return 0;
}

// ---- the wave-per-column allocation kernels: k_zalloc_reg (zalloc_reg.h, N <= 24) and the general LDS-search kernel k_zalloc (kernels.h) ----
// Independent waves, one LDS slab per wave, zacc (and P) shared per workgroup.  The general kernel takes the whole column in one row
// chunk when that leaves room for at least two waves per workgroup, else row chunks of 64 with ZsumG kept in global memory.
struct ZWavePlan {
  bool reg = false;                    // k_zalloc_reg is eligible (N <= ZNMAX and its LDS fits); false: k_zalloc
  ZGeom g{};
  int w = 8, per_cu = 0, grid = 0;     // waves per workgroup, workgroups per CU, workgroups
  size_t lds = 0;
};
static int plan_zwave(size_t K, size_t G, size_t N, bool save_Z, int n_cu, const Switches& sw, ZWavePlan& p) {
  p = ZWavePlan();
  ZGeom& zg = p.g;
  zg.KP = (K % 32 == 0) ? (int)K + 1 : (int)(K | 1);
  zg.HW = (int)((N + 3) / 4);
  zg.TR = N <= 8 ? 8 : N <= 16 ? 16 : N <= 20 ? 20 : 24;   // threshold registers of the k_zalloc_reg instantiation
  p.reg = N <= (size_t)ZNMAX && sw.z_reg;
  size_t slab = 0, shared_words = 0;
  auto geometry = [&](bool chunked) {
    if (p.reg) {
      zg.KC = (int)K;
      slab = (size_t)zg.HW * ZH + (K + 1) * (size_t)zreg_row_words(zg.TR) + 2 * N + N + (save_Z ? N * (size_t)zg.KP : 0);
      zg.zacc_words = (int)((N * (size_t)zg.KP + 3) & ~(size_t)3);
      zg.p_words = (int)((2 * K * N + 3) & ~(size_t)3);                  // workgroup copy of P (fp64)
    } else {
      zg.KC = chunked ? 64 : (int)((K + 63) & ~(size_t)63);
      zg.KP = chunked ? 65 : ((K % 32 == 0) ? (int)K + 1 : (int)(K | 1));
      const bool loc = chunked || save_Z;
      slab = (size_t)zg.HW * ZH + 2 * N + (N - 1) * (size_t)zg.KP + (zg.KC + 1) + zg.KC + N + (loc ? N * (size_t)zg.KP : 0);
      zg.zacc_words = chunked ? 0 : (int)((N * (size_t)zg.KP + 3) & ~(size_t)3);
      zg.p_words = 0;
    }
    slab = (slab + 3) & ~(size_t)3;
    zg.slab_words = (int)slab;
    shared_words = (size_t)zg.zacc_words + zg.p_words;
  };
  // workgroup width.  k_zalloc holds 128 VGPRs per lane: at 16 waves/CU it owns the whole register file and
  // starves k_side (side stream) until its tail.  Measured end to end at the metric config (tools/e2e.py):
  // 16 waves/CU 178 us/iter, 12: 169, 10: 176, 8: 161, 2x4: 165, 6: 179.  So: at most 8 waves per CU, in one
  // workgroup when LDS allows.
  constexpr int Z_MAX_WAVES_PER_CU = 8;
  int best_total = 0;
  auto pick = [&]() {
    p.w = p.per_cu = best_total = 0;
    for (int per_cu = 1; per_cu <= 2; ++per_cu)
      for (int w : {16, 8, 6, 4, 2, 1}) {
        const size_t lds = (shared_words + (size_t)w * slab) * 4;
        if (lds * per_cu <= 160 * 1024 && w * per_cu <= Z_MAX_WAVES_PER_CU && w * per_cu > best_total) { best_total = w * per_cu; p.w = w; p.per_cu = per_cu; }
      }
  };
  geometry(sw.z_chunk && !p.reg);
  pick();
  // the register path keeps (K+1) threshold rows per wave and a workgroup copy of P: for large K (e.g. K = 1,536
  // with N <= 24) that exceeds LDS, so fall back to the general kernel, which can walk the rows in chunks
  if (p.reg && best_total < 2) { p.reg = false; geometry(sw.z_chunk); pick(); }
  if (!p.reg && best_total < 2 && !sw.z_chunk) { geometry(true); pick(); }
  if (sw.zw != ENV_UNSET) { p.w = sw.zw; p.per_cu = (shared_words + (size_t)p.w * slab) * 4 * 2 <= 160 * 1024 ? 2 : 1; }
  if (p.w == 0) return fail(BNMF_EINVAL, "bnmf_create: K = %zu, N = %zu needs %zu B of LDS per wavefront for the allocation kernel (limit 160 KiB): unsupported", K, N, slab * 4);
  p.lds = ((shared_words + (size_t)p.w * slab) * 4 + 15) & ~(size_t)15;
  const long resident = (long)n_cu * p.per_cu;
  const long want = ((long)G + p.w - 1) / p.w;
  p.grid = (int)(want < resident ? want : resident);
  if (sw.z_grid != ENV_UNSET) p.grid = sw.z_grid;          // diagnostics only
  return 0;
}

// ---- the tile kernel k_zalloc_tile (zalloc_tile.h): N > 24 (or K too large for the register kernel), when at least two waves per CU fit ----
struct ZTilePlan {
  bool ok = false, lean = false;       // lean: the register-lean variant, one workgroup of 1024 lanes
  ZTGeom g{};
  int w = 0, grid = 0;                 // waves per workgroup, workgroups
  size_t lds = 0;
};
static ZTilePlan plan_ztile(size_t K, size_t G, size_t N, bool save_Z, int n_cu, const Switches& sw) {
  ZTilePlan p;
  ZTGeom& tg = p.g;
  tg.HW = (int)((N + 3) / 4);
  tg.nch = (int)((K + ZTR - 1) / ZTR);
  tg.p_words = 2 * ztile_np8((int)N) * ZTR;
  tg.zacc_words = (int)((N * (size_t)ZTR + 3) & ~(size_t)3);
  tg.slab_words = (int)ztile_slab_words((int)N, tg.HW, save_Z);
  tg.dbg = nullptr;
  const size_t shw = (size_t)tg.p_words + tg.zacc_words;
  int tper = 0, ttot = 0;
  for (int per_cu = 1; per_cu <= 2; ++per_cu)
    for (int w : {8, 6, 4, 2}) {
      const size_t lds = (shw + (size_t)w * tg.slab_words) * 4;
      // 8 waves per CU: the kernel holds ~190 VGPRs (double-buffered LDS reads), i.e. two waves per SIMD
      if (lds * per_cu <= 160 * 1024 && w * per_cu <= 8 && w * per_cu > ttot) { ttot = w * per_cu; p.w = w; tper = per_cu; }
    }
  // ... or 16 (one workgroup of 1024 lanes) with the register-lean variant, where LDS allows it
  if ((shw + 16 * (size_t)tg.slab_words) * 4 <= 160 * 1024 && !sw.z_nolean) { ttot = 16; p.w = 16; tper = 1; p.lean = true; }
  if (!sw.z_tile || ttot < 2) return p;                    // (BNMF_ZTILE=0: k_zalloc)
  p.ok = true;
  p.lds = ((shw + (size_t)p.w * tg.slab_words) * 4 + 15) & ~(size_t)15;
  // column slices: the fewest rounds (1..4) of resident workgroups that fill >= 97 % of the CUs (the chunk's P rows
  // are staged and its ZsumG counts flushed once per workgroup); every wave with at least two columns
  const long res = (long)n_cu * tper;
  long ns = 1; double best_util = 0.0;
  for (long r = 1; r <= 4; ++r) {
    const long c = (r * res) / tg.nch;
    if (c < 1) continue;
    const double util = (double)(c * tg.nch) / (double)(r * res);
    if (util > best_util + 1e-9) { best_util = util; ns = c; }
    if (util >= 0.97) break;
  }
  const long nsmax = ((long)G + 2 * p.w - 1) / (2 * p.w);
  if (ns > nsmax) ns = nsmax;
  if (ns < 1) ns = 1;
  tg.nslice = (int)ns;
  p.grid = tg.nch * tg.nslice;
  return p;
}

// Static schedule of k_zalloc_sort (zalloc_sort.h): columns dealt into blocks of equal total count (largest column first,
// to the lightest block that still has room), the non-empty cells of a block as items sorted by their number of quads,
// 64 items per task.  M is fixed for the life of the handle, so this runs once.
//
// plan_zsort is the schedule itself: pure host code (no HIP call, no handle), so that its contract can be checked on any machine and for
// any number of CUs (bnmf_test_zsort_plan, tests/test_schedule_host.py); build_zsort uploads what it returns.  p.ok = false: declined.
struct ZSortPlan {
  bool ok = false, it16 = false, pk = false, shared = false;
  int KP = 0, GBc = 0, nb = 0, W = 0, nblk = 0, qmax = 0, nempty = 0;   // nempty: blocks without an own column
  std::vector<ZSBlock> blocks;
  std::vector<int> cols;              // the blocks' columns (own, then guests) in block order, then ONE trailing entry (column 0): see the end of plan_zsort
  std::vector<uint32_t> items;        // 4-byte form, always
  std::vector<uint16_t> items16;      // 2-byte form of the same items, if it16
  std::vector<int32_t> Mblk;
};
static int plan_zsort(const int32_t* M, size_t K, size_t G, size_t N, bool save_Z, int maxM, bool z_reg, int n_cu, const Switches& sw, ZSortPlan& p) {
  p = ZSortPlan();
  if (!z_reg || N > (size_t)ZS_NMAX - 1 || K > 1024) return 0;
  // save_Z: a cell's counts per factor meet as 16-bit halves in k_zexpand's slab
  if (save_Z && maxM > 65535) return 0;
  if (!sw.zsort) return 0;                                                        // diagnostics / tests: the register kernel
  // an item word holds 16 bits of fragment index (k | gl << 10 | f << 16), and f = 65535 with k = 1023, gl = 63 is the empty-lane
  // sentinel: a cell above 65,534 fragments of 4 ZS_QMAX counts stays with the register kernel
  if ((long long)maxM > 65534LL * 4 * ZS_QMAX16) return 0;
  // Round 5: LARGE CELLS ARE SPREAD OVER THE BLOCKS.  A block's work is the counts of its columns, and the columns are dealt whole: a cell of
  // 10^6 counts (six times an average block at the metric configuration) made its block, and with it the launch, six times as long.  The
  // fragments of a cell above ZS_BIG counts beyond its first ZS_HOME are now "exported" in units of ZS_UNIT fragments to the lightest blocks,
  // which host the cell's column as a GUEST column (up to GX extra column slots per block: its A E products, a row of zK); Mhat is still left
  // by the lane of fragment 0, which stays at home.  ZsumK of a column then has several writers: every block adds its share with integer
  // atomics (exact, order-independent) and the draw kernels zero what they have consumed (Dev::zsumk_accum, as for the tile kernel).  Not with
  // save_Z (k_zexpand writes whole columns of Z per block).  The per-count work stays O(sum M) — the reference's rmultinom is O(N) per cell
  // (R/sample_params.R:263) — but a 10^7-count cell is 25 % more counts for the whole chip, not a 60-fold longer block.
  constexpr int ZS_BIG = 8192, ZS_HOME = 16, ZS_UNIT = 32;
  const bool spread = !save_Z && (long long)maxM > ZS_BIG && sw.zs_spread;   // (tests: 0 = every cell at home)
  const int nblk = (int)((N + 4) / 5);                                             // threshold blocks per cell
  const int KP = (K % 32 == 0) ? (int)K + 1 : (int)(K | 1);
  size_t budget = 156 * 1024;                                                     // of 160: the side streams' workgroups (2 KB each) keep room on the CU
  if (sw.zs_lds_kb != ENV_UNSET) budget = (size_t)(long)sw.zs_lds_kb * 1024;
  long nb = std::min<long>((long)G, n_cu);
  int GBc = 0, W = 0;
  for (int tries = 0; tries < 12; ++tries, nb = std::min<long>((long)G, nb * 2)) {
    GBc = (int)((G + nb - 1) / nb);
    if (spread) GBc = std::min(64, GBc + 8);                                      // guest column slots
    if (GBc <= 64 && (long)nb * GBc >= (long)G) {
      const size_t sh = zsort_shared_bytes((int)K, (int)N, KP, GBc, false), wv = zsort_wave_bytes(nblk, (int)N);
      W = 0;
      for (int w : {16, 14, 12, 8, 6, 4}) if (sh + (size_t)w * wv <= budget) { W = w; break; }
      if (W) break;
    }
    if (nb >= (long)G) break;
  }
  if (!W || GBc > 64) return 0;
  { const int w = sw.zs_w; if (w == 4 || w == 6 || w == 8 || w == 12 || w == 14 || w == 16) W = w; }
  // columns -> blocks
  const bool it16_pre = K <= 127 && GBc <= 64 && (long long)maxM <= 8LL * 4 * ZS_QMAX16;
  const int qmax_pre = (it16_pre || (long long)maxM > 65534LL * 4 * ZS_QMAX) ? ZS_QMAX16 : ZS_QMAX;   // quads per fragment (the item format is fixed below: the same rule)
  struct Unit { int g, k, f0, nf; long counts; };
  std::vector<Unit> units;
  std::vector<long> ctot(G, 0), cfull(G, 0);
  for (size_t g = 0; g < G; ++g) {
    long sacc = 0, exported = 0;
    for (size_t k = 0; k < K; ++k) {
      const long m = M[k + K * g];
      sacc += m;
      if (spread && m > ZS_BIG) {
        const long qt = (m + 3) >> 2, F = (qt + qmax_pre - 1) / qmax_pre;
        for (long f0 = ZS_HOME; f0 < F; f0 += ZS_UNIT) {
          const long nf = std::min<long>(ZS_UNIT, F - f0);
          const long cnt = std::min<long>(m, (f0 + nf) * 4L * qmax_pre) - f0 * 4L * qmax_pre;
          units.push_back({(int)g, (int)k, (int)f0, (int)nf, cnt});
          exported += cnt;
        }
      }
    }
    cfull[g] = sacc; ctot[g] = sacc - exported;
  }
  std::vector<int> order(G);
  for (size_t g = 0; g < G; ++g) order[g] = (int)g;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ctot[a] > ctot[b]; });
  std::vector<std::vector<int>> bcols(nb);
  std::vector<long> bload(nb, 0);
  const int own_cap = spread ? std::max(1, (int)((G + nb - 1) / nb)) : GBc;        // own columns per block (the rest of GBc: guest slots)
  {
    // min-heap of (load, block) over the blocks that still have room
    std::vector<std::pair<long, int>> heap;
    for (int b = 0; b < nb; ++b) heap.push_back({0L, b});
    auto cmp = [](const std::pair<long, int>& a, const std::pair<long, int>& b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (int g : order) {
      std::pop_heap(heap.begin(), heap.end(), cmp);
      auto top = heap.back(); heap.pop_back();
      bcols[top.second].push_back(g);
      top.first += ctot[g];
      if ((int)bcols[top.second].size() < own_cap) { heap.push_back(top); std::push_heap(heap.begin(), heap.end(), cmp); }
    }
  }
  for (int b = 0; b < nb; ++b) { std::sort(bcols[b].begin(), bcols[b].end()); long l = 0; for (int g : bcols[b]) l += ctot[g]; bload[b] = l; }
  // the exported units -> the lightest blocks (largest unit first); a block takes a unit if it owns the column, hosts it already, or has a
  // guest slot left; a unit nobody can take stays with its column's owner
  std::vector<std::vector<int>> gcols(nb);                                         // guest columns per block, in slot order
  struct BUnit { int k, gl, f0, nf; };
  std::vector<std::vector<BUnit>> bunits(nb);
  if (!units.empty()) {
    std::vector<int> owner(G, -1);
    for (int b = 0; b < nb; ++b) for (int g : bcols[b]) owner[g] = b;
    std::stable_sort(units.begin(), units.end(), [](const Unit& a, const Unit& b) { return a.counts > b.counts; });
    std::vector<std::pair<long, int>> heap;
    for (int b = 0; b < nb; ++b) heap.push_back({bload[b], b});
    auto cmp = [](const std::pair<long, int>& a, const std::pair<long, int>& b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    auto slot_of = [&](int b, int g, bool take) -> int {
      if (owner[g] == b) return (int)(std::lower_bound(bcols[b].begin(), bcols[b].end(), g) - bcols[b].begin());
      for (size_t i = 0; i < gcols[b].size(); ++i) if (gcols[b][i] == g) return (int)(bcols[b].size() + i);
      if (take && (int)(bcols[b].size() + gcols[b].size()) < GBc) { gcols[b].push_back(g); return (int)(bcols[b].size() + gcols[b].size() - 1); }
      return -1;
    };
    for (const Unit& u : units) {
      std::vector<std::pair<long, int>> skipped;
      int dst = -1, gl = -1;
      for (int tries = 0; tries < 16 && !heap.empty(); ++tries) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        auto top = heap.back(); heap.pop_back();
        gl = slot_of(top.second, u.g, true);
        if (gl >= 0) { dst = top.second; top.first += u.counts; heap.push_back(top); std::push_heap(heap.begin(), heap.end(), cmp); break; }
        skipped.push_back(top);
      }
      for (auto& x : skipped) { heap.push_back(x); std::push_heap(heap.begin(), heap.end(), cmp); }
      if (dst < 0) {                                                               // home: its load grows (the heap entry is found and raised)
        dst = owner[u.g]; gl = slot_of(dst, u.g, false);
        for (auto& x : heap) if (x.second == dst) x.first += u.counts;
        std::make_heap(heap.begin(), heap.end(), cmp);
      }
      bunits[dst].push_back({u.k, gl, u.f0, u.nf});
    }
  }
  // Quads per item.  Round 5 (end): chosen per data set where no cell is large enough to be spread.  A wave alone with its task runs a quad in
  // ~0.33 us (one dependent chain; tools/zstamps.py, tools/zsmall.py) and the waves of a SIMD share its issue at about twice that per wave
  // and quad: with few cells per block (K = 96, G = 2,000: 13 tasks for 14 waves) the kernel WAS its largest task — 64 quads with 2-byte
  // items, 20 of its 34 us.  Estimated per block in quad units, T = 6 for a task's thresholds: max(T + largest item, 2 (quads / 64 + T tasks)
  // / W); the candidate with the smallest worst block wins, the larger one on a near-tie (fewer items, fewer thresholds).  Measured, device
  // time of the kernel in us at K = 96, N = 20 with 64 / 32 / 16 / 8 / 4 quads per item: G = 250: 35.1 / 24.8 / 19.6 / 16.9 / 16.3; 1,000: 35.8 /
  // 25.3 / 20.2 / 19.6 / 21.2; 2,000: 36.2 / 26.5 / 23.3 / 24.0 / 29.1; 4,000: 37.2 / 31.6 / 30.1 / 34.0 / 44.1; 10,000: 52.7 / 53.4 / 56.7 / 69.0 /
  // 94.1.  The draws do not depend on it (Philox counter = cell, count index).  BNMF_ZSQMAX: tests.
  int qsel = 0;
  if (!spread && (long long)maxM <= ZS_BIG) {          // (above: the fragment index of a 4-byte item is 16 bits)
    const int cand[5] = {64, 32, 16, 8, 4};
    double worst[5] = {0, 0, 0, 0, 0};
    for (int b = 0; b < nb; ++b) {
      long Q = 0, I[5] = {0, 0, 0, 0, 0}; int maxqt = 0;
      for (int g : bcols[b]) for (size_t k = 0; k < K; ++k) {
        const int m = M[k + K * (size_t)g], qt = m > 0 ? (m + 3) >> 2 : 0;
        Q += qt; maxqt = std::max(maxqt, qt);
        for (int c = 0; c < 5; ++c) I[c] += qt ? (qt + cand[c] - 1) / cand[c] : 1;
      }
      for (int c = 0; c < 5; ++c) {
        const double est = std::max(6.0 + std::min(cand[c], maxqt), 2.0 * ((double)Q / 64.0 + 6.0 * (double)((I[c] + 63) / 64)) / (double)W);
        worst[c] = std::max(worst[c], est);
      }
    }
    double best = 1e300;
    for (int c = 0; c < 5; ++c) if (worst[c] < 0.95 * best) { best = worst[c]; qsel = cand[c]; }
    { const int v = sw.zs_qmax; if (v == 4 || v == 8 || v == 16 || v == 32 || v == 64) qsel = v; }
  }
  // 2-byte items where row, column-in-block and fragment index fit 7 + 6 + 3 bits (and 0xFFFF stays free for the empty lane)
  bool it16 = K <= 127 && GBc <= 64 && (long long)maxM <= 8LL * 4 * (qsel ? qsel : ZS_QMAX16);
  it16 = it16 && sw.zs_it16;                                                        // diagnostics / tests: 0 = 4-byte items
  // (large cells spread over the blocks: 4-byte items of 128 counts per fragment, 256 where a cell would need more than 65,534 of them)
  const int qmax = qsel ? qsel : (it16 || (long long)maxM > 65534LL * 4 * ZS_QMAX) ? ZS_QMAX16 : ZS_QMAX;
  std::vector<ZSBlock> blocks(nb);
  std::vector<int> cols;
  std::vector<uint32_t> items;
  // two factors per word in the block's zG / zK tables (16-bit halves): only if no half can overflow, i.e. every column total
  // (bound of a ZsumK entry) and every row total over a block's columns (bound of the block's share of a ZsumG entry) < 2^16
  bool pk = *std::max_element(cfull.begin(), cfull.end()) < 65536;                  // (the WHOLE column: units of a large cell may be dealt back to its owner)
  // the blocks are independent: their item lists are built by a few host threads (the schedule was 20 of the 50 ms of bnmf_create
  // at the metric configuration)
  std::vector<std::vector<uint32_t>> bitems(nb);
  std::vector<char> bpk(nb, 1);
  auto build_blocks = [&](long b0, long b1) {
    std::vector<std::pair<int, uint32_t>> tmp;
    for (long b = b0; b < b1; ++b) {
      for (size_t k = 0; k < K && bpk[b]; ++k) {
        long r = 0;
        for (int g : bcols[b]) r += M[k + K * (size_t)g];
        for (int g : gcols[b]) r += M[k + K * (size_t)g];                          // (a guest column's share: bounded by the whole cell)
        if (r >= 65536) bpk[b] = 0;
      }
      tmp.clear();
      for (size_t gl = 0; gl < bcols[b].size(); ++gl) {
        const size_t g = (size_t)bcols[b][gl];
        for (size_t k = 0; k < K; ++k) {
          const int m = M[k + K * g];
          if (m <= 0) { tmp.push_back({0, (uint32_t)k | ((uint32_t)gl << 10)}); continue; }   // an item without counts: its lane leaves Mhat of the cell (s.mh)
          const int qt = (m + 3) >> 2;
          const int fend = (spread && m > ZS_BIG) ? ZS_HOME : INT_MAX;                // a large cell: the fragments beyond the first ZS_HOME are units (below, or in other blocks)
          for (int f = 0; f * qmax < qt && f < fend; ++f)
            tmp.push_back({std::min(qmax, qt - f * qmax), (uint32_t)k | ((uint32_t)gl << 10) | ((uint32_t)f << 16)});
        }
      }
      for (const BUnit& u : bunits[b]) {                                             // units of large cells this block works on (its own columns' or guests')
        const size_t g = u.gl < (int)bcols[b].size() ? (size_t)bcols[b][u.gl] : (size_t)gcols[b][u.gl - (int)bcols[b].size()];
        const int m = M[u.k + K * g], qt = (m + 3) >> 2;
        for (int f = u.f0; f < u.f0 + u.nf && f * qmax < qt; ++f)
          tmp.push_back({std::min(qmax, qt - f * qmax), (uint32_t)u.k | ((uint32_t)u.gl << 10) | ((uint32_t)f << 16)});
      }
      std::stable_sort(tmp.begin(), tmp.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
      // inside a task (64 consecutive items) the order is free: ascending row, so that neighbouring lanes read neighbouring
      // rows of the LDS copy of P and add to neighbouring words of the block's ZsumG table (few bank conflicts)
      for (size_t i0 = 0; i0 < tmp.size(); i0 += 64)
        std::sort(tmp.begin() + i0, tmp.begin() + std::min(tmp.size(), i0 + 64), [](const auto& a, const auto& b) { return (a.second & 1023u) < (b.second & 1023u); });
      std::vector<uint32_t>& it = bitems[b];
      it.reserve(tmp.size() + 64);
      for (const auto& x : tmp) it.push_back(x.second);
      while (it.size() % 64) it.push_back(0xFFFFFFFFu);
    }
  };
  {
    const long nthr = std::max<long>(1, std::min<long>({(long)std::thread::hardware_concurrency(), 16L, nb}));
    std::vector<std::thread> pool;
    for (long i = 1; i < nthr; ++i) pool.emplace_back(build_blocks, nb * i / nthr, nb * (i + 1) / nthr);
    build_blocks(0, nb / nthr);
    for (auto& th : pool) th.join();
  }
  for (int b = 0; b < nb; ++b) pk = pk && bpk[b];
  pk = pk && sw.zs_pk;                                                              // diagnostics / tests: 0 = one factor per word
  // the waves per workgroup were sized for one factor per word (the block tables' larger form); with two per word the tables are half as
  // large and, at the metric configuration, 14 waves fit where 12 did.  tools/ablong.py, sixteen processes alternating on one box: 12 waves
  // 80.3 us per iteration in three of eight processes and 81.4-83.0 in the others (the stop-event mode of DESIGN.md 5b), 14 waves 81.3-81.6
  // in seven of eight (80.3 in one): 82.1 against 81.3 us on average
  if (pk && sw.zs_w == ENV_UNSET) {
    const size_t sh = zsort_shared_bytes((int)K, (int)N, KP, GBc, true), wv = zsort_wave_bytes(nblk, (int)N);
    for (int w : {16, 14, 12, 8, 6, 4}) if (sh + (size_t)w * wv <= budget) { W = std::max(W, w); break; }
  }
  std::vector<int32_t> Mblk(K * G);
  for (int b = 0; b < nb; ++b) {
    ZSBlock& bk = blocks[b];
    bk.item0 = (int)items.size(); bk.col0 = (int)cols.size(); bk.ncols = (int)(bcols[b].size() + gcols[b].size());
    items.insert(items.end(), bitems[b].begin(), bitems[b].end());
    bk.ntask = (int)(bitems[b].size() / 64);
    for (int pass = 0; pass < 2; ++pass)
      for (int g : (pass ? gcols[b] : bcols[b])) {
        if (Mblk.size() < K * (cols.size() + 1)) Mblk.resize(K * (cols.size() + 1));
        memcpy(Mblk.data() + K * cols.size(), M + K * (size_t)g, K * sizeof(int32_t)); cols.push_back(g);
      }
  }
  if (items.empty()) items.push_back(0xFFFFFFFFu);
  if (it16) {
    p.items16.resize(items.size());
    for (size_t i = 0; i < items.size(); ++i) {
      const uint32_t v = items[i];
      p.items16[i] = v == 0xFFFFFFFFu ? (uint16_t)0xFFFFu : (uint16_t)((v & 127u) | (((v >> 10) & 63u) << 7) | ((v >> 16) << 13));
    }
  }
  // WHAT A KERNEL MAY READ OF A BLOCK WITHOUT COLUMNS.  All-zero columns add no load: they pile onto the lightest block until it is full, and
  // with G between one and two times the number of blocks and most columns empty the last blocks get none (ncols = 0, col0 = the length of
  // the list; the exported units of large cells go to exactly those blocks, as guests).  The set-up of k_zalloc_sort reads cols[col0 + 0] for
  // the lanes beyond its block's A E products, whatever ncols is, and E of that column (the product is discarded): cols[col0 .. col0 +
  // max(ncols, 1)) must be inside the list and name real columns.  Hence one trailing entry, column 0, which no block owns through it.
  cols.push_back(0);
  for (int b = 0; b < nb; ++b) p.nempty += bcols[b].empty() ? 1 : 0;
  p.ok = true; p.it16 = it16; p.pk = pk; p.shared = !units.empty();
  p.KP = KP; p.GBc = GBc; p.nb = (int)nb; p.W = W; p.nblk = nblk; p.qmax = qmax;
  p.blocks.swap(blocks); p.cols.swap(cols); p.items.swap(items); p.Mblk.swap(Mblk);
  return 0;
}

// Static schedule of k_zalloc_step (zalloc_step.h): columns dealt to the workgroups by total count (largest first, to the
// lightest workgroup that still has room), a workgroup's columns cut into batches of <= GBP, a batch's rows into chunks of
// 32; the cells of a step (chunk x batch) as items — zero-count cells too: their Mhat feeds the metric terms — sorted by
// their number of quads (counting sort) and dealt to the workgroup's waves in snake order, 64 per task: the waves of a step
// get the same number of items of the same sizes.  M is fixed for the life of the handle, so this runs once.
//
// plan_zstep / build_zstep: the schedule as pure host code, and its upload (as plan_zsort / build_zsort).  Every workgroup has a column:
// a column costs its counts plus a fixed 64 K, so a workgroup without one is lighter than any with one and is dealt to first.
struct ZStepPlan {
  bool ok = false, it16 = false;
  int nch = 0, nwg = 0, W = 0, GBP = 0, L = 0, maxfrag = 0;
  std::vector<ZPWg> wgs;
  std::vector<ZPBatch> batches;
  std::vector<ZPStep> steps;
  std::vector<int> cols;
  std::vector<uint32_t> items;        // 4-byte form, always
  std::vector<uint16_t> items16;      // 2-byte form of the same items, if it16
};
static int plan_zstep(const int32_t* M, size_t K, size_t G, size_t N, bool save_Z, int n_cu, const Switches& sw, ZStepPlan& p) {
  p = ZStepPlan();
  if (save_Z || N <= (size_t)ZNMAX || N > (size_t)ZP_NMAX) return 0;
  if (!sw.zstep) return 0;                                                         // diagnostics / tests: the tile kernel
  const int L = 4;                                                                 // lanes per cell (with <= 20 included factors the search then skips a level)
  size_t budget = 156 * 1024;                                                      // of 160: the side streams' workgroups keep room on the CU
  int GBP = 0, W = 0;
  // 8 waves (two per SIMD).  12 waves fit the LDS up to N = 60 and were measured at config 4: 114.5 against 121 us per launch, but
  // at the 168 registers three waves per SIMD leave, the kernel spills 16-36 bytes per lane — not kept
  for (int gbp : {40, 32}) if (zstep_shared_bytes((int)N, gbp) + 8 * zstep_wave_bytes(L) <= budget) { GBP = gbp; W = 8; break; }
  if (sw.zp_gb == 32 || sw.zp_gb == 40) GBP = sw.zp_gb;                            // diagnostics / tests
  if (!GBP) return 0;
  const int nch = (int)((K + ZP_KC - 1) / ZP_KC);
  const long nwg = std::min<long>((long)G, n_cu);
  // columns -> workgroups
  std::vector<long> ctot(G, 0);
  for (size_t g = 0; g < G; ++g) { long sacc = 0; for (size_t k = 0; k < K; ++k) sacc += M[k + K * g]; ctot[g] = sacc; }
  std::vector<int> order(G);
  for (size_t g = 0; g < G; ++g) order[g] = (int)g;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ctot[a] > ctot[b]; });
  const size_t cap = (G + nwg - 1) / nwg + 2;                                      // the threshold work of a column does not depend on its counts
  std::vector<std::vector<int>> wcols(nwg);
  {
    std::vector<std::pair<long, int>> heap;
    for (int b = 0; b < nwg; ++b) heap.push_back({0L, b});
    auto cmp = [](const std::pair<long, int>& a, const std::pair<long, int>& b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (int g : order) {
      std::pop_heap(heap.begin(), heap.end(), cmp);
      auto top = heap.back(); heap.pop_back();
      wcols[top.second].push_back(g);
      top.first += ctot[g] + 64 * (long)K;                                         // + the cells' fixed cost (Mhat, thresholds), in counts
      if (wcols[top.second].size() < cap) { heap.push_back(top); std::push_heap(heap.begin(), heap.end(), cmp); }
    }
  }
  std::vector<ZPWg> wgs(nwg);
  std::vector<ZPBatch> batches;
  std::vector<int> cols;
  for (int b = 0; b < nwg; ++b) {
    std::sort(wcols[b].begin(), wcols[b].end());
    const int nc = (int)wcols[b].size(), nb = (nc + GBP - 1) / GBP;
    wgs[b] = ZPWg{(int)batches.size(), nb};
    for (int i = 0; i < nb; ++i) {
      const int c0 = (int)((long)nc * i / nb), c1 = (int)((long)nc * (i + 1) / nb);
      batches.push_back(ZPBatch{(int)cols.size(), c1 - c0});
      for (int x = c0; x < c1; ++x) cols.push_back(wcols[b][x]);
    }
  }
  std::vector<ZPStep> steps(batches.size() * (size_t)nch);
  std::vector<uint32_t> items;
  items.reserve((size_t)((double)K * (double)G * 1.05) + 64 * steps.size());
  std::vector<uint32_t> bucket[ZP_QMAX + 1], wlist[ZP_WMAX], sorted;
  int maxfrag = 0;
  for (size_t bi = 0; bi < batches.size(); ++bi) {
    const ZPBatch& bt = batches[bi];
    for (int ch = 0; ch < nch; ++ch) {
      const size_t k0 = (size_t)ch * ZP_KC, kc = std::min<size_t>(ZP_KC, K - k0);
      for (auto& v : bucket) v.clear();
      for (int gl = 0; gl < bt.ncols; ++gl) {
        const size_t g = (size_t)cols[bt.col0 + gl];
        for (size_t kl = 0; kl < kc; ++kl) {
          const int m = M[k0 + kl + K * g];
          const int qt = m > 0 ? (m + 3) >> 2 : 0;
          const uint32_t base = (uint32_t)kl | ((uint32_t)gl << 5);
          if (qt == 0) { bucket[0].push_back(base); continue; }
          for (int f = 0; f * ZP_QMAX < qt; ++f) {
            if (f >= (1 << 21)) return fail(BNMF_EINVAL, "bnmf_create: a cell of M holds %d counts: unsupported", m);
            bucket[std::min(ZP_QMAX, qt - f * ZP_QMAX)].push_back(base | ((uint32_t)f << 11));
            maxfrag = std::max(maxfrag, f);
          }
        }
      }
      // sorted by size, then dealt to the waves in snake order: every wave gets the same number of items (+-1) of the same sizes
      sorted.clear();
      for (int qn = ZP_QMAX; qn >= 0; --qn) sorted.insert(sorted.end(), bucket[qn].begin(), bucket[qn].end());
      for (int w = 0; w < W; ++w) wlist[w].clear();
      for (size_t i = 0; i < sorted.size(); ++i) { const int r = (int)(i % (2 * (size_t)W)); wlist[r < W ? r : 2 * W - 1 - r].push_back(sorted[i]); }
      size_t mx = 0;
      for (int w = 0; w < W; ++w) mx = std::max(mx, wlist[w].size());
      ZPStep& st = steps[bi * (size_t)nch + ch];
      st.item0 = (long long)items.size(); st.pad = 0;
      st.ntw = (int)((mx + 63) / 64);
      for (int w = 0; w < W; ++w) { const auto& v = wlist[w]; items.insert(items.end(), v.begin(), v.end()); items.insert(items.end(), (size_t)st.ntw * 64 - v.size(), 0xFFFFFFFFu); }
    }
  }
  if (items.empty()) items.push_back(0xFFFFFFFFu);
  // 2-byte items where the fragment index fits 5 bits beside row (5) and column (6), 0xFFFF staying the empty lane (column 63 does not
  // occur): BNMF_ZPIT16=0 keeps the 4-byte form (diagnostics / tests)
  const bool it16 = maxfrag <= 30 && sw.zp_it16;
  if (it16) {
    p.items16.resize(items.size());
    for (size_t i = 0; i < items.size(); ++i) p.items16[i] = items[i] == 0xFFFFFFFFu ? (uint16_t)0xFFFFu : (uint16_t)items[i];
  }
  p.ok = true; p.it16 = it16; p.nch = nch; p.nwg = (int)nwg; p.W = W; p.GBP = GBP; p.L = L; p.maxfrag = maxfrag;
  p.wgs.swap(wgs); p.batches.swap(batches); p.steps.swap(steps); p.cols.swap(cols); p.items.swap(items);
  return 0;
}
