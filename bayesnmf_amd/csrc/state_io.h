// bayesnmf_amd/csrc/state_io.h — a chain's state in a file and back (bnmf_save_state, bnmf_load_state, bnmf_state_info).
// Host code only, included at the end of api.hip: it reads the handle's buffers through the same helpers the sweep uses.
//
// File (little-endian, no pointers, no time stamps, every reserved field zero: the same chain saved twice gives the same bytes):
//   header   128 B  "BNMFSTAT", format version, header size, the bnmf_config without device / temperature pointer, a hash of the data
//                   as the handle holds it (int32 counts, or fp64 for Normal) and of the temperature schedule, zeros, checksum of the above
//   records         "BNMFREC1", since_iter, iter, number of sections, 0, payload bytes; the sections; checksum of header and payload.
//                   since_iter = 0: a full record (the first of a file); S > 0: a delta on top of the record that ended at iteration S.
//   section   32 B  kind, id, first iteration (rings), element count, element size, 0; then count * size bytes of data
// What a record holds and what it leaves to the next bnmf_run: DESIGN.md §10.

namespace {

constexpr uint32_t ST_VERSION = 1;
constexpr size_t ST_HDR = 128, ST_RHDR = 32, ST_SHDR = 32;
constexpr size_t ST_STAGE = (size_t)32 << 20;        // each of the two pinned staging halves
enum { SEC_HYPER = 1, SEC_ARRAY = 2, SEC_R = 3, SEC_ZSUMK = 4, SEC_ZSUMG = 5, SEC_Z = 6, SEC_ZREC = 7, SEC_RING = 8, SEC_ZRING = 9,
       SEC_ZRECRING = 10, SEC_HIST = 11, SEC_FIXED = 12 /* the mask of fixed columns of P: base record only, only if a column is fixed */ };

// 64-bit word hash (multiply-xorshift), streamed: the data hash of a handle, the temperature hash and the checksums
struct Hash64 {
  uint64_t h = 0x9E3779B97F4A7C15ull, n = 0;
  unsigned char pend[8]; int np = 0;
  void word(uint64_t w) { h = (h ^ w) * 0x9FB21C651E98DF25ull; h ^= h >> 31; }
  void update(const void* p, size_t len) {
    const unsigned char* c = (const unsigned char*)p;
    n += len;
    while (np && len) { pend[np++] = *c++; --len; if (np == 8) { uint64_t w; memcpy(&w, pend, 8); word(w); np = 0; } }
    for (; len >= 8; c += 8, len -= 8) { uint64_t w; memcpy(&w, c, 8); word(w); }
    while (len) { pend[np++] = *c++; --len; }
  }
  uint64_t final() const {
    Hash64 t = *this;
    if (t.np) { uint64_t w = 0; memcpy(&w, t.pend, (size_t)t.np); t.word(w); }
    t.word(t.n);
    return t.h ^ (t.h >> 29);
  }
};
uint64_t hash_bytes(const void* p, size_t len) { Hash64 x; x.update(p, len); return x.final(); }

// little-endian field packing into a byte buffer (no struct padding reaches the file)
struct Pack {
  std::vector<unsigned char> b;
  template <class T> void put(T v) { unsigned char t[sizeof(T)]; memcpy(t, &v, sizeof(T)); b.insert(b.end(), t, t + sizeof(T)); }
  void raw(const void* p, size_t n) { b.insert(b.end(), (const unsigned char*)p, (const unsigned char*)p + n); }
};
template <class T> T get_at(const unsigned char* p, size_t off) { T v; memcpy(&v, p + off, sizeof(T)); return v; }

struct StHeader {
  int32_t K, G, N, likelihood, prior, MH, learning_rank, rank_method, save_Z, window;
  uint64_t seed; uint32_t chain_id; int64_t n_temperature; uint64_t data_hash, temp_hash;
};
std::vector<unsigned char> header_bytes(const StHeader& s) {
  Pack p;
  p.raw("BNMFSTAT", 8); p.put<uint32_t>(ST_VERSION); p.put<uint32_t>((uint32_t)ST_HDR);
  for (int32_t v : {s.K, s.G, s.N, s.likelihood, s.prior, s.MH, s.learning_rank, s.rank_method, s.save_Z, s.window}) p.put<int32_t>(v);
  p.put<uint64_t>(s.seed); p.put<uint32_t>(s.chain_id); p.put<uint32_t>(0);
  p.put<int64_t>(s.n_temperature); p.put<uint64_t>(s.data_hash); p.put<uint64_t>(s.temp_hash);
  p.b.resize(ST_HDR - 8, 0);
  p.put<uint64_t>(hash_bytes(p.b.data(), p.b.size()));
  return p.b;
}
StHeader handle_header(const bnmf_handle* h) {
  const bnmf_config& c = h->cfg;
  return StHeader{c.K, c.G, c.N, c.likelihood, c.prior, c.MH, c.learning_rank, c.rank_method, c.save_Z, c.window, c.seed, c.chain_id,
                  (int64_t)h->temp_host.size(), h->data_hash, hash_bytes(h->temp_host.data(), h->temp_host.size() * sizeof(double))};
}
// header: magic, version, checksum; *out filled
int parse_header(const char* fn, const char* path, const unsigned char* b, size_t got, StHeader* out) {
  if (got < ST_HDR) return fail(BNMF_EINVAL, "%s: %s is not a chain state file (%zu bytes, shorter than its header)", fn, path, got);
  if (memcmp(b, "BNMFSTAT", 8) != 0) return fail(BNMF_EINVAL, "%s: %s is not a chain state file (bad magic)", fn, path);
  const uint32_t ver = get_at<uint32_t>(b, 8);
  if (ver != ST_VERSION) return fail(BNMF_EINVAL, "%s: %s has format version %u, this library reads version %u", fn, path, ver, ST_VERSION);
  if (get_at<uint32_t>(b, 12) != ST_HDR || get_at<uint64_t>(b, ST_HDR - 8) != hash_bytes(b, ST_HDR - 8))
    return fail(BNMF_EINVAL, "%s: %s: the file header is corrupt (checksum)", fn, path);
  int32_t v[10];
  for (int i = 0; i < 10; ++i) v[i] = get_at<int32_t>(b, 16 + 4 * i);
  *out = StHeader{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], get_at<uint64_t>(b, 56), get_at<uint32_t>(b, 64),
                  get_at<int64_t>(b, 72), get_at<uint64_t>(b, 80), get_at<uint64_t>(b, 88)};
  return 0;
}
// every field a loader must agree on, named in the refusal
int match_header(const char* fn, const StHeader& f, const StHeader& w) {
  struct { const char* name; long long file, handle; } rows[] = {
      {"K", f.K, w.K}, {"G", f.G, w.G}, {"N", f.N, w.N}, {"likelihood", f.likelihood, w.likelihood}, {"prior", f.prior, w.prior},
      {"MH", f.MH, w.MH}, {"learning_rank", f.learning_rank, w.learning_rank}, {"rank_method", f.rank_method, w.rank_method},
      {"save_Z", f.save_Z, w.save_Z}, {"window", f.window, w.window}, {"chain_id", f.chain_id, w.chain_id},
      {"n_temperature", f.n_temperature, w.n_temperature}};
  for (const auto& r : rows)
    if (r.file != r.handle) return fail(BNMF_EINVAL, "%s: the file's chain has %s = %lld, the handle %lld", fn, r.name, r.file, r.handle);
  if (f.seed != w.seed) return fail(BNMF_EINVAL, "%s: the file's chain has seed = %llu, the handle %llu", fn, (unsigned long long)f.seed, (unsigned long long)w.seed);
  if (f.data_hash != w.data_hash) return fail(BNMF_EINVAL, "%s: the file was saved from other data (data hash %016llx, the handle's %016llx)", fn,
                                              (unsigned long long)f.data_hash, (unsigned long long)w.data_hash);
  if (f.temp_hash != w.temp_hash) return fail(BNMF_EINVAL, "%s: the file was saved with another temperature schedule", fn);
  return 0;
}

// one section of a record: where its bytes live on the device (up to two runs: a ring that wraps) or on the host
struct Sec {
  uint32_t kind; int32_t id; int64_t first; int64_t count; uint32_t esize;
  const void* run_p[2] = {nullptr, nullptr}; size_t run_n[2] = {0, 0};   // device runs (bytes)
  std::vector<unsigned char> host;                                        // host-side data (R, scalars, hist)
  size_t bytes() const { return (size_t)count * esize; }
};
size_t ring_runs(size_t wcap, int64_t first, int64_t ns, size_t slot_bytes, const void* base, const void** p, size_t* n) {
  const size_t s0 = (size_t)((first - 1) % (int64_t)wcap), n1 = std::min<size_t>((size_t)ns, wcap - s0);
  p[0] = (const unsigned char*)base + s0 * slot_bytes; n[0] = n1 * slot_bytes;
  p[1] = base; n[1] = ((size_t)ns - n1) * slot_bytes;
  return n[1] ? 2 : 1;
}
// the iterations of the rings a record carries: the kept ones, [max(1, iter - window + 1), iter], after since_iter
void kept_range(const bnmf_handle* h, int since, int64_t* first, int64_t* ns) {
  const int64_t lo = std::max<int64_t>({1, (int64_t)h->iter - h->cfg.window + 1, (int64_t)since + 1});
  *first = lo; *ns = std::max<int64_t>(0, (int64_t)h->iter - lo + 1);
}
// the current value of every array the model records (P, E, A, its prior parameters, acceptance rates, sigmasq; R goes as an integer)
std::vector<int> state_ids(const bnmf_handle* h) {
  std::vector<int> ids = recorded_ids(h);
  ids.erase(std::remove(ids.begin(), ids.end(), (int)BNMF_R), ids.end());
  return ids;
}
int plan_record(bnmf_handle* h, int since, std::vector<Sec>& out) {
  const size_t K = h->cfg.K, G = h->cfg.G, N = h->cfg.N;
  out.clear();
  auto dev = [](uint32_t kind, int id, int64_t count, uint32_t es, const void* p) { Sec s{kind, id, 0, count, es}; s.run_p[0] = p; s.run_n[0] = (size_t)count * es; return s; };
  if (since == 0)                                              // hyper-prior values: the base record only (they never change)
    for (int id = 0; id < BNMF_ID_MAX; ++id) {
      const Arr& a = h->arr[id];
      if (!is_hyper(id) || !a.d) continue;
      out.push_back(dev(SEC_HYPER, id, a.stride == 0 ? 1 : (int64_t)id_len(h, id), 8, a.d));
    }
  if (since == 0 && h->n_fixed > 0) {                         // (a chain without fixed columns writes the bytes it always wrote)
    Sec s{SEC_FIXED, BNMF_P, 0, (int64_t)N, 4};
    s.host.resize(N * 4); memcpy(s.host.data(), h->fixedP.data(), N * 4);
    out.push_back(s);
  }
  for (int id : state_ids(h)) {
    const Arr& a = h->arr[id];
    if (!a.d) return fail(BNMF_ESTATE, "bnmf_save_state: array id %d has no value", id);
    const size_t len = id_len(h, id);
    out.push_back(dev(SEC_ARRAY, id, (int64_t)len, 8, a.d + (is_prior_param(id) ? (size_t)cur_slot(h) * len : 0)));
  }
  { int r = 0; HIPCHK(hipMemcpy(&r, h->dR, sizeof(int), hipMemcpyDeviceToHost)); Sec s{SEC_R, BNMF_R, 0, 1, 4}; s.host.resize(4); memcpy(s.host.data(), &r, 4); out.push_back(s); }
  if (h->cfg.likelihood == BNMF_POISSON) {                     // the Gibbs draws of the next iteration read them
    out.push_back(dev(SEC_ZSUMK, BNMF_ZSUMK, (int64_t)(N * G), 4, h->dZsumK));
    out.push_back(dev(SEC_ZSUMG, BNMF_ZSUMG, (int64_t)(K * N), 4, h->dZsumG));
  }
  if (h->dZ) {
    if (int rc = ensure_Z(h)) return rc;                       // (the sorted schedule keeps Z as records: expanded for the file)
    out.push_back(dev(SEC_Z, BNMF_Z, (int64_t)(K * N * G), 4, h->dZ));
    if (h->zs.dRec && !h->zs.dRecRing) out.push_back(dev(SEC_ZREC, 0, (int64_t)h->zs.recwords, 4, h->zs.dRec));
  }
  int64_t first = 0, ns = 0;
  kept_range(h, since, &first, &ns);
  if (h->wcap > 0 && ns > 0) {
    for (int id : recorded_ids(h)) {
      const Arr& a = h->arr[id];
      if (!a.ring) continue;
      const size_t len = id_len(h, id);
      Sec s{SEC_RING, id, first, ns * (int64_t)len, 8};
      ring_runs((size_t)h->wcap, first, ns, len * 8, a.ring, s.run_p, s.run_n);
      out.push_back(s);
    }
    if (h->zring) {
      const size_t len = id_len(h, BNMF_Z);
      Sec s{SEC_ZRING, BNMF_Z, first, ns * (int64_t)len, 4};
      ring_runs((size_t)h->wcap, first, ns, len * 4, h->zring, s.run_p, s.run_n);
      out.push_back(s);
    }
    if (h->zs.dRecRing) {
      Sec s{SEC_ZRECRING, 0, first, ns * (int64_t)h->zs.recwords, 4};
      ring_runs((size_t)h->wcap, first, ns, h->zs.recwords * 4, h->zs.dRecRing, s.run_p, s.run_n);
      out.push_back(s);
    }
  }
  if (h->wcap > 0) {
    Sec s{SEC_HIST, 0, 0, (int64_t)h->hist.size(), 8};
    s.host.resize(h->hist.size() * 8); memcpy(s.host.data(), h->hist.data(), s.host.size());
    out.push_back(s);
  }
  return 0;
}

// Two pinned halves on the handle: the device side of chunk i + 1 is in flight while chunk i is written / read on the host
int ensure_stage(bnmf_handle* h) {
  if (h->hStage) return 0;
  HIPCHK(hipHostMalloc((void**)&h->hStage, 2 * ST_STAGE, hipHostMallocDefault));
  return 0;
}
struct Events { hipEvent_t e[2] = {nullptr, nullptr}; ~Events() { for (auto x : e) if (x) hipEventDestroy(x); } };

int fwrite_all(FILE* f, const void* p, size_t n, Hash64& hs) {
  hs.update(p, n);
  if (n && fwrite(p, 1, n, f) != n) return fail(BNMF_EINVAL, "bnmf_save_state: write failed (%s)", strerror(errno));
  return 0;
}
std::vector<unsigned char> sec_header(const Sec& s) {
  Pack p;
  p.put<uint32_t>(s.kind); p.put<int32_t>(s.id); p.put<int64_t>(s.first); p.put<int64_t>(s.count); p.put<uint32_t>(s.esize); p.put<uint32_t>(0);
  return p.b;
}
int write_record(bnmf_handle* h, FILE* f, int since, const std::vector<Sec>& secs, size_t* bytes) {
  size_t payload = 0;
  for (const Sec& s : secs) payload += ST_SHDR + s.bytes();
  Pack r;
  r.raw("BNMFREC1", 8); r.put<int32_t>(since); r.put<int32_t>(h->iter); r.put<uint32_t>((uint32_t)secs.size()); r.put<uint32_t>(0);
  r.put<uint64_t>((uint64_t)payload);
  Hash64 hs;
  if (int rc = fwrite_all(f, r.b.data(), r.b.size(), hs)) return rc;
  if (int rc = ensure_stage(h)) return rc;
  Events ev;
  HIPCHK(hipEventCreateWithFlags(&ev.e[0], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&ev.e[1], hipEventDisableTiming));
  for (const Sec& s : secs) {
    const auto sh = sec_header(s);
    if (int rc = fwrite_all(f, sh.data(), sh.size(), hs)) return rc;
    if (!s.host.empty() || s.bytes() == 0) { if (int rc = fwrite_all(f, s.host.data(), s.host.size(), hs)) return rc; continue; }
    // the section's device bytes in chunks of ST_STAGE, alternating halves: issue chunk i + 1, then write chunk i
    struct Ch { const unsigned char* p; size_t n; };
    std::vector<Ch> ch;
    for (int r2 = 0; r2 < 2; ++r2)
      for (size_t o = 0; o < s.run_n[r2]; o += ST_STAGE) ch.push_back({(const unsigned char*)s.run_p[r2] + o, std::min(ST_STAGE, s.run_n[r2] - o)});
    auto issue = [&](size_t i) -> int {
      HIPCHK(hipMemcpyAsync(h->hStage + (i & 1) * ST_STAGE, ch[i].p, ch[i].n, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipEventRecord(ev.e[i & 1], h->stream));
      return 0;
    };
    if (!ch.empty()) if (int rc = issue(0)) return rc;
    for (size_t i = 0; i < ch.size(); ++i) {
      if (i + 1 < ch.size()) if (int rc = issue(i + 1)) return rc;
      HIPCHK(hipEventSynchronize(ev.e[i & 1]));
      if (int rc = fwrite_all(f, h->hStage + (i & 1) * ST_STAGE, ch[i].n, hs)) return rc;
    }
  }
  const uint64_t sum = hs.final();
  if (fwrite(&sum, 1, 8, f) != 8) return fail(BNMF_EINVAL, "bnmf_save_state: write failed (%s)", strerror(errno));
  *bytes = r.b.size() + payload + 8;
  return 0;
}

struct RecInfo { long off; int since, iter; uint32_t nsec; uint64_t payload; };
// Walk a file: header, then every record.  check = true: every record's checksum and section headers are verified (read in full);
// false: only the record headers are read (bnmf_save_state's delta check).  h (may be null): its config must match, and every
// section must fit its buffers.
int scan_file(const char* fn, const char* path, FILE* f, const bnmf_handle* h, bool check, StHeader* hdr, std::vector<RecInfo>& recs, long* fsize) {
  recs.clear();
  if (fseek(f, 0, SEEK_END) != 0) return fail(BNMF_EINVAL, "%s: %s: cannot seek", fn, path);
  *fsize = ftell(f);
  rewind(f);
  unsigned char hb[ST_HDR];
  const size_t got = fread(hb, 1, ST_HDR, f);
  if (int rc = parse_header(fn, path, hb, got, hdr)) return rc;
  if (h) if (int rc = match_header(fn, *hdr, handle_header(h))) return rc;
  std::vector<unsigned char> buf(check ? ST_STAGE : 0);
  long off = (long)ST_HDR;
  int prev_iter = 0;
  while (off < *fsize) {
    const int ri = (int)recs.size();
    unsigned char rb[ST_RHDR];
    if (*fsize - off < (long)ST_RHDR || fseek(f, off, SEEK_SET) != 0 || fread(rb, 1, ST_RHDR, f) != ST_RHDR)
      return fail(BNMF_EINVAL, "%s: %s: record %d is truncated (its header)", fn, path, ri);
    if (memcmp(rb, "BNMFREC1", 8) != 0) return fail(BNMF_EINVAL, "%s: %s: record %d is corrupt (bad record tag)", fn, path, ri);
    RecInfo r{off, get_at<int32_t>(rb, 8), get_at<int32_t>(rb, 12), get_at<uint32_t>(rb, 16), get_at<uint64_t>(rb, 24)};
    if (get_at<uint32_t>(rb, 20) != 0 || r.iter < 1 || r.since < 0 || r.since > r.iter)
      return fail(BNMF_EINVAL, "%s: %s: record %d is corrupt (header fields)", fn, path, ri);
    if ((uint64_t)(*fsize - off) < ST_RHDR + r.payload + 8)
      return fail(BNMF_EINVAL, "%s: %s: record %d (iteration %d) is truncated: %llu bytes announced, %ld left", fn, path, ri, r.iter,
                  (unsigned long long)(ST_RHDR + r.payload + 8), *fsize - off);
    if (ri == 0 && r.since != 0) return fail(BNMF_EINVAL, "%s: %s: the first record is a delta (since iteration %d), not a full record", fn, path, r.since);
    if (ri > 0 && r.since != prev_iter)
      return fail(BNMF_EINVAL, "%s: %s: record %d is not contiguous: a delta since iteration %d follows a record at iteration %d", fn, path, ri, r.since, prev_iter);
    if (check) {
      Hash64 hs;
      hs.update(rb, ST_RHDR);
      uint64_t left = r.payload;
      uint32_t nsec = 0;
      while (left > 0) {                                       // section headers, then their data through the buffer
        unsigned char sb[ST_SHDR];
        if (left < ST_SHDR || fread(sb, 1, ST_SHDR, f) != ST_SHDR) return fail(BNMF_EINVAL, "%s: %s: record %d (iteration %d) is corrupt (section layout)", fn, path, ri, r.iter);
        hs.update(sb, ST_SHDR); left -= ST_SHDR; ++nsec;
        const uint32_t kind = get_at<uint32_t>(sb, 0), es = get_at<uint32_t>(sb, 24);
        const int64_t count = get_at<int64_t>(sb, 16);
        if (kind < SEC_HYPER || kind > SEC_FIXED || (es != 4 && es != 8) || count < 0 || (uint64_t)count * es > left || get_at<uint32_t>(sb, 28) != 0)
          return fail(BNMF_EINVAL, "%s: %s: record %d (iteration %d) is corrupt (section %u)", fn, path, ri, r.iter, nsec - 1);
        uint64_t n = (uint64_t)count * es;
        left -= n;
        while (n > 0) {
          const size_t c = (size_t)std::min<uint64_t>(n, buf.size());
          if (fread(buf.data(), 1, c, f) != c) return fail(BNMF_EINVAL, "%s: %s: record %d (iteration %d) is truncated", fn, path, ri, r.iter);
          hs.update(buf.data(), c); n -= c;
        }
      }
      uint64_t sum = 0;
      if (nsec != r.nsec || fread(&sum, 1, 8, f) != 8 || sum != hs.final())
        return fail(BNMF_EINVAL, "%s: %s: record %d (iterations %d..%d) is corrupt: bad checksum", fn, path, ri, r.since + 1, r.iter);
    }
    recs.push_back(r);
    prev_iter = r.iter;
    off += (long)(ST_RHDR + r.payload + 8);
  }
  if (recs.empty()) return fail(BNMF_EINVAL, "%s: %s holds no record", fn, path);
  return 0;
}
struct FileCloser { FILE* f; ~FileCloser() { if (f) fclose(f); } };

// a section as the handle must take it: its device destination (up to two runs), or 0 with an error naming the mismatch
int sec_dest(bnmf_handle* h, int ri, int iter, uint32_t kind, int id, int64_t first, int64_t count, uint32_t es, void** p, size_t* n) {
  const size_t K = h->cfg.K, G = h->cfg.G, N = h->cfg.N;
  p[0] = p[1] = nullptr; n[0] = n[1] = 0;
  auto bad = [&](const char* what) { return fail(BNMF_EINVAL, "bnmf_load_state: record %d (iteration %d): %s (section kind %u, id %d)", ri, iter, what, kind, id); };
  auto one = [&](void* d, size_t want, uint32_t wes) { if ((size_t)count != want || es != wes) return bad("size does not match the handle"); p[0] = d; n[0] = want * wes; return 0; };
  switch (kind) {
    case SEC_HYPER: {
      if (id < 0 || id >= BNMF_ID_MAX || !is_hyper(id) || es != 8 || (count != 1 && (size_t)count != id_len(h, id))) return bad("not a hyper-prior value of this handle");
      return 0;                                                // (set through bnmf_set_array by the caller)
    }
    case SEC_ARRAY: {
      const auto ids = state_ids(h);
      if (std::find(ids.begin(), ids.end(), id) == ids.end()) return bad("not a state array of this model");
      const size_t len = id_len(h, id);
      return one(nullptr, len, 8);                             // (the array is allocated when the record is applied)
    }
    case SEC_R: return one(h->dR, 1, 4);
    case SEC_ZSUMK: return one(h->dZsumK, N * G, 4);
    case SEC_ZSUMG: return one(h->dZsumG, K * N, 4);
    case SEC_Z: if (!h->dZ) return bad("Z in the file, save_Z off in the handle"); return one(h->dZ, K * N * G, 4);
    case SEC_ZREC: if (!h->zs.dRec || h->zs.dRecRing) return bad("Z records the handle does not keep"); return one(h->zs.dRec, h->zs.recwords, 4);
    case SEC_HIST: if (h->wcap <= 0) return bad("a history without a window"); return one(nullptr, (size_t)h->wcap * 4, 8);
    case SEC_FIXED: if (id != BNMF_P || ri != 0) return bad("a mask of fixed columns outside the base record, or not of P"); return one(nullptr, N, 4);
    case SEC_RING: case SEC_ZRING: case SEC_ZRECRING: {
      const int64_t lo = std::max<int64_t>(1, (int64_t)iter - h->cfg.window + 1);
      size_t slot = 0; void* base = nullptr; uint32_t wes = 8;
      if (kind == SEC_RING) {
        const auto rids = recorded_ids(h);
        if (id < 0 || id >= BNMF_ID_MAX || std::find(rids.begin(), rids.end(), id) == rids.end() || !h->arr[id].ring) return bad("a ring this handle does not record");
        slot = id_len(h, id); base = h->arr[id].ring;
      } else if (kind == SEC_ZRING) {
        if (!h->zring) return bad("a Z ring this handle does not keep");
        slot = id_len(h, BNMF_Z); base = h->zring; wes = 4;
      } else {
        if (!h->zs.dRecRing) return bad("a ring of Z records this handle does not keep");
        slot = h->zs.recwords; base = h->zs.dRecRing; wes = 4;
      }
      if (es != wes || slot == 0 || count % (int64_t)slot != 0) return bad("ring section size does not match the handle");
      const int64_t ns = count / (int64_t)slot;
      if (ns < 1 || first < lo || first + ns - 1 > iter) return bad("ring samples outside the record's kept iterations");
      const void* cp[2]; ring_runs((size_t)h->wcap, first, ns, slot * wes, base, cp, n);
      p[0] = (void*)cp[0]; p[1] = (void*)cp[1];
      return 0;
    }
  }
  return bad("unknown section");
}

// every section of every record fits the handle, and the full record carries every state array (before any device write)
int check_sections(bnmf_handle* h, const char* path, FILE* f, const std::vector<RecInfo>& recs) {
  const auto ids = state_ids(h);
  std::vector<int> have;
  std::vector<int32_t> file_mask;
  for (size_t ri = 0; ri < recs.size(); ++ri) {
    long off = recs[ri].off + (long)ST_RHDR;
    for (uint32_t i = 0; i < recs[ri].nsec; ++i) {
      unsigned char sb[ST_SHDR];
      if (fseek(f, off, SEEK_SET) != 0 || fread(sb, 1, ST_SHDR, f) != ST_SHDR) return fail(BNMF_EINVAL, "bnmf_load_state: record %zu: cannot read a section", ri);
      void* p[2]; size_t n[2];
      const uint32_t kind = get_at<uint32_t>(sb, 0), es = get_at<uint32_t>(sb, 24);
      const int64_t count = get_at<int64_t>(sb, 16);
      if (int rc = sec_dest(h, (int)ri, recs[ri].iter, kind, get_at<int32_t>(sb, 4), get_at<int64_t>(sb, 8), count, es, p, n)) return rc;
      if (kind == SEC_FIXED) {                                 // a mask given to the handle beforehand must be the file's
        file_mask.resize((size_t)count);
        if (fread(file_mask.data(), 4, (size_t)count, f) != (size_t)count) return fail(BNMF_EINVAL, "bnmf_load_state: record %zu: cannot read a section", ri);
        for (int32_t v : file_mask) if (v != 0 && v != 1) return fail(BNMF_EINVAL, "bnmf_load_state: %s: the mask of fixed columns is corrupt", path);
      }
      if (kind == SEC_ARRAY && ri == 0) have.push_back(get_at<int32_t>(sb, 4));
      if (kind == SEC_R && ri == 0) have.push_back(BNMF_R);
      off += (long)(ST_SHDR + (size_t)count * es);
    }
  }
  for (int id : ids) if (std::find(have.begin(), have.end(), id) == have.end())
    return fail(BNMF_EINVAL, "bnmf_load_state: %s: the full record carries no value of array id %d", path, id);
  if (std::find(have.begin(), have.end(), (int)BNMF_R) == have.end()) return fail(BNMF_EINVAL, "bnmf_load_state: %s: the full record carries no R", path);
  if (!h->fixedP.empty())
    for (size_t n = 0; n < h->fixedP.size(); ++n) {
      const int32_t fv = file_mask.empty() ? 0 : file_mask[n];
      if (fv != h->fixedP[n])
        return fail(BNMF_ESTATE, "bnmf_load_state: column %zu of P is %s in %s and %s on the handle (bnmf_set_fixed)", n, fv ? "fixed" : "not fixed", path,
                    h->fixedP[n] ? "fixed" : "not fixed");
    }
  return 0;
}

}  // namespace

static uint64_t state_data_hash(const void* p, size_t bytes) { return hash_bytes(p, bytes); }

extern "C" {

int bnmf_save_state(bnmf_handle* h, const char* path, int since_iter, size_t* bytes_written) {
  if (!h || !path) return fail(BNMF_EINVAL, "bnmf_save_state: null argument");
  if (h->poisoned) return fail(BNMF_ESTATE, "bnmf_save_state: the handle timed out inside a kernel; its state is not the chain's");
  if (!h->inited) return fail(BNMF_ESTATE, "bnmf_save_state: the handle has no state yet (call bnmf_init or bnmf_load_state first)");
  if (since_iter < 0 || since_iter > h->iter) return fail(BNMF_EINVAL, "bnmf_save_state: since_iter = %d outside [0, iter = %d]", since_iter, h->iter);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->side));
  HIPCHK(hipStreamSynchronize(h->side2));
  FileCloser fc{nullptr};
  long old_size = 0;
  if (since_iter == 0) {
    fc.f = fopen(path, "wb");
    if (!fc.f) return fail(BNMF_EINVAL, "bnmf_save_state: cannot create %s (%s)", path, strerror(errno));
    const auto hb = header_bytes(handle_header(h));
    if (fwrite(hb.data(), 1, hb.size(), fc.f) != hb.size()) return fail(BNMF_EINVAL, "bnmf_save_state: write failed (%s)", strerror(errno));
  } else {
    fc.f = fopen(path, "r+b");
    if (!fc.f) return fail(BNMF_EINVAL, "bnmf_save_state: a delta needs the existing file %s (%s)", path, strerror(errno));
    StHeader hdr; std::vector<RecInfo> recs;
    if (int rc = scan_file("bnmf_save_state", path, fc.f, h, false, &hdr, recs, &old_size)) return rc;
    if (recs.back().iter != since_iter)
      return fail(BNMF_EINVAL, "bnmf_save_state: %s ends at iteration %d, not at since_iter = %d", path, recs.back().iter, since_iter);
    if (fseek(fc.f, old_size, SEEK_SET) != 0) return fail(BNMF_EINVAL, "bnmf_save_state: cannot seek in %s", path);
  }
  std::vector<Sec> secs;
  size_t bytes = 0;
  int rc = plan_record(h, since_iter, secs);
  if (!rc) rc = write_record(h, fc.f, since_iter, secs, &bytes);
  if (!rc && fflush(fc.f) != 0) rc = fail(BNMF_EINVAL, "bnmf_save_state: write failed (%s)", strerror(errno));
  if (rc) {                                                    // a delta that failed half-way: the file ends where it ended before
    char keep[sizeof g_err]; memcpy(keep, g_err, sizeof keep);
    if (since_iter > 0) { fflush(fc.f); if (ftruncate(fileno(fc.f), old_size) != 0) {} }
    memcpy(g_err, keep, sizeof keep);
    return rc;
  }
  if (bytes_written) *bytes_written = bytes + (since_iter == 0 ? ST_HDR : 0);
  return 0;
}

int bnmf_load_state(bnmf_handle* h, const char* path, int* iter_out) {
  if (!h || !path) return fail(BNMF_EINVAL, "bnmf_load_state: null argument");
  if (h->poisoned) return fail(BNMF_ESTATE, "bnmf_load_state: the handle timed out inside a kernel; destroy it");
  if (h->inited || h->iter != 0) return fail(BNMF_ESTATE, "bnmf_load_state: the handle has already run (iteration %d); load into a handle fresh from bnmf_create", h->iter);
  FileCloser fc{fopen(path, "rb")};
  if (!fc.f) return fail(BNMF_EINVAL, "bnmf_load_state: cannot open %s (%s)", path, strerror(errno));
  StHeader hdr; std::vector<RecInfo> recs; long fsize = 0;
  if (int rc = scan_file("bnmf_load_state", path, fc.f, h, true, &hdr, recs, &fsize)) return rc;
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ensure_rings(h)) return rc;                     // (allocations only: the rings' slots are written below)
  if (int rc = check_sections(h, path, fc.f, recs)) return rc;
  // the file is sound and fits: replay it
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->side));
  HIPCHK(hipStreamSynchronize(h->side2));
  if (int rc = ensure_stage(h)) return rc;
  Events ev;
  HIPCHK(hipEventCreateWithFlags(&ev.e[0], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&ev.e[1], hipEventDisableTiming));
  struct IterGuard { bnmf_handle* h; bool done = false; ~IterGuard() { if (!done) h->iter = 0; } } guard{h};   // a replay that fails: not "has run"
  bool have_ev[2] = {false, false};
  size_t half = 0;
  std::vector<int32_t> file_mask;                              // applied once the replay has succeeded: a failed one leaves the handle's mask alone
  for (size_t ri = 0; ri < recs.size(); ++ri) {
    const int iter = recs[ri].iter;
    h->iter = iter;                                            // (cur_slot: the prior parameters of this record's iteration)
    long off = recs[ri].off + (long)ST_RHDR;
    for (uint32_t i = 0; i < recs[ri].nsec; ++i) {
      unsigned char sb[ST_SHDR];
      if (fseek(fc.f, off, SEEK_SET) != 0 || fread(sb, 1, ST_SHDR, fc.f) != ST_SHDR) return fail(BNMF_EINVAL, "bnmf_load_state: %s: read failed", path);
      const uint32_t kind = get_at<uint32_t>(sb, 0), es = get_at<uint32_t>(sb, 24);
      const int id = get_at<int32_t>(sb, 4);
      const int64_t count = get_at<int64_t>(sb, 16);
      const size_t nbytes = (size_t)count * es;
      off += (long)(ST_SHDR + nbytes);
      void* p[2]; size_t n[2];
      if (int rc = sec_dest(h, (int)ri, iter, kind, id, get_at<int64_t>(sb, 8), count, es, p, n)) return rc;
      if (kind == SEC_FIXED) {
        file_mask.resize((size_t)count);
        if (fread(file_mask.data(), 1, nbytes, fc.f) != nbytes) return fail(BNMF_EINVAL, "bnmf_load_state: %s: read failed", path);
        continue;
      }
      if (kind == SEC_HYPER || kind == SEC_HIST) {             // small: through host memory
        std::vector<double> v((size_t)count);
        if (fread(v.data(), 1, nbytes, fc.f) != nbytes) return fail(BNMF_EINVAL, "bnmf_load_state: %s: read failed", path);
        if (kind == SEC_HIST) h->hist = v;
        else if (int rc = bnmf_set_array(h, id, v.data(), v.size())) return rc;
        continue;
      }
      if (kind == SEC_ARRAY) {
        if (int rc = ensure(h, id)) return rc;
        const size_t len = id_len(h, id);
        p[0] = h->arr[id].d + (is_prior_param(id) ? (size_t)cur_slot(h) * len : 0); n[0] = nbytes;
        h->arr[id].n = len; h->arr[id].stride = 1;
      }
      // file -> pinned half -> device, alternating halves: the read of chunk i + 1 overlaps the copy of chunk i
      for (int r2 = 0; r2 < 2; ++r2)
        for (size_t o = 0; o < n[r2]; o += ST_STAGE) {
          const size_t c = std::min(ST_STAGE, n[r2] - o);
          if (have_ev[half]) HIPCHK(hipEventSynchronize(ev.e[half]));
          unsigned char* st = h->hStage + half * ST_STAGE;
          if (fread(st, 1, c, fc.f) != c) return fail(BNMF_EINVAL, "bnmf_load_state: %s: read failed", path);
          HIPCHK(hipMemcpyAsync((unsigned char*)p[r2] + o, st, c, hipMemcpyHostToDevice, h->stream));
          HIPCHK(hipEventRecord(ev.e[half], h->stream));
          have_ev[half] = true; half ^= 1;
        }
    }
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!file_mask.empty()) if (int rc = apply_fixed(h, file_mask.data())) return rc;
  // What the next bnmf_run recomputes (the hyper sweep of iter + 1, Esum / Psum, Et, nzE, Mhat, the partial sums) is invalidated as
  // bnmf_init's re-initialisation does it; the sync words are cleared — a handle from the pool may hold another chain's
  HIPCHK(hipMemset(h->dFlags, 0, 64));
  memset(h->hErr, 0, 64);
  if (h->rank.dSync) HIPCHK(hipMemset(h->rank.dSync, 0, 32));
  if (h->rank.dCol) HIPCHK(hipMemset(h->rank.dCol, 0, (size_t)RK_REP * 4 * 2 * (((size_t)h->cfg.G + RK_MAXC - 1) / RK_MAXC) * sizeof(double)));
  HIPCHK(hipMemset(h->dDrawOwn, 0, (size_t)h->cfg.N * sizeof(unsigned)));
  h->draw_seq = 0;
  h->pipe = Pipe{};
  h->pipe.z_expanded_iter = h->dZ ? h->iter : 0;                   // (the file's Z is the current iteration's)
  if (h->wcap > 0 && h->hist.size() != (size_t)h->wcap * 4) h->hist.assign((size_t)h->wcap * 4, std::nan(""));
  refresh_dev(h);
  h->inited = true;
  guard.done = true;
  if (iter_out) *iter_out = h->iter;
  return 0;
}

int bnmf_state_info(const char* path, bnmf_state_desc* out) {
  if (!path || !out) return fail(BNMF_EINVAL, "bnmf_state_info: null argument");
  FileCloser fc{fopen(path, "rb")};
  if (!fc.f) return fail(BNMF_EINVAL, "bnmf_state_info: cannot open %s (%s)", path, strerror(errno));
  StHeader hdr; std::vector<RecInfo> recs; long fsize = 0;
  if (int rc = scan_file("bnmf_state_info", path, fc.f, nullptr, true, &hdr, recs, &fsize)) return rc;
  memset(out, 0, sizeof *out);
  out->K = hdr.K; out->G = hdr.G; out->N = hdr.N; out->likelihood = hdr.likelihood; out->prior = hdr.prior; out->MH = hdr.MH;
  out->learning_rank = hdr.learning_rank; out->rank_method = hdr.rank_method; out->save_Z = hdr.save_Z; out->window = hdr.window;
  out->seed = hdr.seed; out->chain_id = hdr.chain_id; out->format_version = (int32_t)ST_VERSION; out->n_temperature = hdr.n_temperature;
  out->data_hash = hdr.data_hash; out->temperature_hash = hdr.temp_hash;
  out->first_iter = recs.front().iter; out->last_iter = recs.back().iter; out->n_records = (int32_t)recs.size();
  out->bytes = (int64_t)fsize;
  return 0;
}

}  // extern "C"
