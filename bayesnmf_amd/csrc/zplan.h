// bayesnmf_amd/csrc/zplan.h — the static schedules of k_zalloc_sort and k_zalloc_step as pure host code: no HIP call, no handle.
// Included by api.hip (one translation unit); build_zsort / build_zstep there upload what these return, bnmf_test_zsort_plan /
// bnmf_test_zstep_plan hand it to tests/test_schedule_host.py on any machine.

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
static int plan_zsort(const int32_t* M, size_t K, size_t G, size_t N, bool save_Z, int maxM, bool z_reg, int n_cu, ZSortPlan& p) {
  p = ZSortPlan();
  if (!z_reg || N > (size_t)ZS_NMAX - 1 || K > 1024) return 0;
  // save_Z: a cell's counts per factor meet as 16-bit halves in k_zexpand's slab
  if (save_Z && maxM > 65535) return 0;
  if (const char* e = getenv("BNMF_ZSORT")) if (atoi(e) == 0) return 0;          // diagnostics / tests: the register kernel
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
  const bool spread = !save_Z && (long long)maxM > ZS_BIG && !(getenv("BNMF_ZSSPREAD") && atoi(getenv("BNMF_ZSSPREAD")) == 0);   // (tests: 0 = every cell at home)
  const int nblk = (int)((N + 4) / 5);                                             // threshold blocks per cell
  const int KP = (K % 32 == 0) ? (int)K + 1 : (int)(K | 1);
  size_t budget = 156 * 1024;                                                     // of 160: the side streams' workgroups (2 KB each) keep room on the CU
  if (const char* e = getenv("BNMF_ZSLDS")) budget = (size_t)atol(e) * 1024;
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
  if (const char* e = getenv("BNMF_ZSW")) { const int w = atoi(e); if (w == 4 || w == 6 || w == 8 || w == 12 || w == 14 || w == 16) W = w; }
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
    if (const char* e = getenv("BNMF_ZSQMAX")) { const int v = atoi(e); if (v == 4 || v == 8 || v == 16 || v == 32 || v == 64) qsel = v; }
  }
  // 2-byte items where row, column-in-block and fragment index fit 7 + 6 + 3 bits (and 0xFFFF stays free for the empty lane)
  bool it16 = K <= 127 && GBc <= 64 && (long long)maxM <= 8LL * 4 * (qsel ? qsel : ZS_QMAX16);
  if (const char* e = getenv("BNMF_ZSIT16")) it16 = it16 && atoi(e) != 0;           // diagnostics / tests: 0 = 4-byte items
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
  if (const char* e = getenv("BNMF_ZSPK")) pk = pk && atoi(e) != 0;                 // diagnostics / tests: 0 = one factor per word
  // the waves per workgroup were sized for one factor per word (the block tables' larger form); with two per word the tables are half as
  // large and, at the metric configuration, 14 waves fit where 12 did.  tools/ablong.py, sixteen processes alternating on one box: 12 waves
  // 80.3 us per iteration in three of eight processes and 81.4-83.0 in the others (the stop-event mode of DESIGN.md 5b), 14 waves 81.3-81.6
  // in seven of eight (80.3 in one): 82.1 against 81.3 us on average
  if (pk && !getenv("BNMF_ZSW")) {
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
static int plan_zstep(const int32_t* M, size_t K, size_t G, size_t N, bool save_Z, int n_cu, ZStepPlan& p) {
  p = ZStepPlan();
  if (save_Z || N <= (size_t)ZNMAX || N > (size_t)ZP_NMAX) return 0;
  if (const char* e = getenv("BNMF_ZSTEP")) if (atoi(e) == 0) return 0;            // diagnostics / tests: the tile kernel
  const int L = 4;                                                                 // lanes per cell (with <= 20 included factors the search then skips a level)
  size_t budget = 156 * 1024;                                                      // of 160: the side streams' workgroups keep room on the CU
  int GBP = 0, W = 0;
  // 8 waves (two per SIMD).  12 waves fit the LDS up to N = 60 and were measured at config 4: 114.5 against 121 us per launch, but
  // at the 168 registers three waves per SIMD leave, the kernel spills 16-36 bytes per lane — not kept
  for (int gbp : {40, 32}) if (zstep_shared_bytes((int)N, gbp) + 8 * zstep_wave_bytes(L) <= budget) { GBP = gbp; W = 8; break; }
  if (const char* e = getenv("BNMF_ZPGB")) { const int v = atoi(e); if (v == 32 || v == 40) GBP = v; }   // diagnostics / tests
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
  const bool it16 = maxfrag <= 30 && !(getenv("BNMF_ZPIT16") && atoi(getenv("BNMF_ZPIT16")) == 0);
  if (it16) {
    p.items16.resize(items.size());
    for (size_t i = 0; i < items.size(); ++i) p.items16[i] = items[i] == 0xFFFFFFFFu ? (uint16_t)0xFFFFu : (uint16_t)items[i];
  }
  p.ok = true; p.it16 = it16; p.nch = nch; p.nwg = (int)nwg; p.W = W; p.GBP = GBP; p.L = L; p.maxfrag = maxfrag;
  p.wgs.swap(wgs); p.batches.swap(batches); p.steps.swap(steps); p.cols.swap(cols); p.items.swap(items);
  return 0;
}
