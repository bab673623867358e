// tools/subtypes_reduce_check.cpp — bnmf_subtypes' finish (csrc/reduce_host.h: subtypes_finish with con_rows and con_canon64) as a
// stand-alone host program, so that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o subtypes_reduce_check tools/subtypes_reduce_check.cpp
//   subtypes_reduce_check in.bin out.bin
// in.bin: int64 m, G, N, C, Sm, Q; double min_certainty; int32 members [m], query [Q], labs [Sm][m] (the matched samples' labels in member
// order, -1 = unassigned), sizes [Sm][C]; doubles cen [Sm][N*C].  The whole-number counts that the device forms from the labels are formed
// here the same way.  out.bin, all doubles: membership [C][G], label [G], tumour [3][G], centre [4][N*C], size [4][C], together [Q][G],
// then n_included, n_left_out, n_certain, n_never_assigned, mean_certainty, least_certain, least_certain_at, smallest_subtype,
// smallest_subtype_at; the same again with every output NULL must give the same info (checked here).  tests/test_subtypes_host.py builds
// it, runs it and holds out.bin to the numpy restatement bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t hd[6]; double min_certainty;
  if (std::fread(hd, 8, 6, f) != 6 || std::fread(&min_certainty, 8, 1, f) != 1 || hd[0] < 1 || hd[1] < hd[0] || hd[2] < 1 || hd[3] < 2 || hd[3] > BNMF_SUB_MAX_C ||
      hd[4] < 2 || hd[5] < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
  const long m = (long)hd[0], G = (long)hd[1]; const int N = (int)hd[2], C = (int)hd[3], Sm = (int)hd[4], Q = (int)hd[5];
  const size_t NC = (size_t)N * C;
  std::vector<int> members(m);
  std::vector<int32_t> query(Q), labs((size_t)Sm * m), sizes((size_t)Sm * C);
  std::vector<double> cen((size_t)Sm * NC);
  auto get = [&](void* p, size_t size, size_t n) { return n == 0 || std::fread(p, size, n, f) == n; };   // (an empty vector has no address to read to)
  if (!get(members.data(), 4, members.size()) || !get(query.data(), 4, query.size()) || !get(labs.data(), 4, labs.size()) || !get(sizes.data(), 4, sizes.size()) ||
      !get(cen.data(), 8, cen.size())) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);
  std::vector<long> place(G, -1);
  for (long i = 0; i < m; ++i) {
    if (members[i] < 0 || members[i] >= G || (i && members[i] <= members[i - 1])) { std::fprintf(stderr, "bad member list\n"); return 2; }
    place[members[i]] = i;
  }
  for (int32_t v : query) if (v < 0 || v >= G || place[v] < 0) { std::fprintf(stderr, "bad query\n"); return 2; }
  for (int32_t v : labs) if (v < -1 || v >= C) { std::fprintf(stderr, "bad label\n"); return 2; }
  // k_sub_count's counts
  std::vector<int32_t> cnt((size_t)C * m, 0), asg(m, 0), tog((size_t)Q * m, 0), both((size_t)Q * m, 0);
  for (int s = 0; s < Sm; ++s)
    for (long i = 0; i < m; ++i) {
      const int32_t l = labs[(size_t)s * m + i];
      if (l >= 0) { ++asg[i]; ++cnt[(size_t)l * m + i]; }
      for (int q = 0; q < Q; ++q) {
        const int32_t lq = labs[(size_t)s * m + place[query[q]]];
        both[(size_t)q * m + i] += (lq >= 0 && l >= 0) ? 1 : 0;
        tog[(size_t)q * m + i] += (lq >= 0 && lq == l) ? 1 : 0;
      }
    }
  std::vector<double> mem((size_t)C * G), tu(3 * (size_t)G), ce(4 * NC), sz(4 * (size_t)C), tg((size_t)Q * G);
  std::vector<int32_t> lab(G);
  bnmf_subtypes_info a, b;
  std::memset(&a, 0, sizeof a); std::memset(&b, 0, sizeof b);
  const int32_t* qp = Q ? query.data() : nullptr;
  subtypes_finish(members.data(), m, G, N, C, Sm, cnt.data(), asg.data(), Q, qp, tog.data(), both.data(), cen.data(), sizes.data(), min_certainty, mem.data(),
                  lab.data(), tu.data(), ce.data(), sz.data(), Q ? tg.data() : nullptr, &a);
  subtypes_finish(members.data(), m, G, N, C, Sm, cnt.data(), asg.data(), Q, qp, tog.data(), both.data(), cen.data(), sizes.data(), min_certainty, nullptr, nullptr,
                  nullptr, nullptr, nullptr, nullptr, &b);
  if (std::memcmp(&a, &b, sizeof a) != 0) { std::fprintf(stderr, "the info depends on the optional outputs\n"); return 1; }
  std::vector<double> out(mem);
  out.insert(out.end(), lab.begin(), lab.end());
  out.insert(out.end(), tu.begin(), tu.end());
  out.insert(out.end(), ce.begin(), ce.end());
  out.insert(out.end(), sz.begin(), sz.end());
  out.insert(out.end(), tg.begin(), tg.end());
  for (double v : {(double)a.n_included, (double)a.n_left_out, (double)a.n_certain, (double)a.n_never_assigned, a.mean_certainty, a.least_certain,
                   (double)a.least_certain_at, a.smallest_subtype, (double)a.smallest_subtype_at}) out.push_back(v);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  std::fwrite(out.data(), 8, out.size(), o);
  std::fclose(o);
  return 0;
}
