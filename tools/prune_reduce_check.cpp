// tools/prune_reduce_check.cpp — bnmf_prune's finish (csrc/reduce_host.h: prune_finish with con_canon64) as a stand-alone host program, so
// that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o prune_reduce_check tools/prune_reduce_check.cpp
//   prune_reduce_check in.bin out.bin
// in.bin: int64 m, G, N, S; int32 members [m]; doubles mm [m], ld [4][N*m], tum [7][m], trials [m], ser [2][S] (what the device leaves: the
// rows in member order, the whole-number sums of trials, the series' sums).  out.bin, all doubles: load [4][N*G], tumour [7][G], series
// [2][S], signature [3][N], then n_included, n_undefined, n_single, trials, max_change; the same again with every optional output NULL must
// give the same info and series (checked here).  tests/test_prune_host.py builds it, runs it and holds out.bin to the numpy restatement
// bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t hd[4];
  if (std::fread(hd, 8, 4, f) != 4 || hd[0] < 1 || hd[1] < hd[0] || hd[2] < 1 || hd[2] > BNMF_PRN_MAX_N || hd[3] < 1) { std::fprintf(stderr, "bad header\n"); return 2; }
  const long m = (long)hd[0], G = (long)hd[1]; const int N = (int)hd[2], S = (int)hd[3];
  const size_t Nm = (size_t)N * m, NG = (size_t)N * G;
  std::vector<int> members(m);
  std::vector<double> mm(m), ld(4 * Nm), tum(7 * (size_t)m), tr(m), ser(2 * (size_t)S);
  auto get = [&](void* p, size_t size, size_t n) { return std::fread(p, size, n, f) == n; };
  if (!get(members.data(), 4, members.size()) || !get(mm.data(), 8, mm.size()) || !get(ld.data(), 8, ld.size()) || !get(tum.data(), 8, tum.size()) ||
      !get(tr.data(), 8, tr.size()) || !get(ser.data(), 8, ser.size())) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);
  for (long i = 0; i < m; ++i)
    if (members[i] < 0 || members[i] >= G || (i && members[i] <= members[i - 1])) { std::fprintf(stderr, "bad member list\n"); return 2; }
  std::vector<double> load(4 * NG), tu(7 * (size_t)G), sig(3 * (size_t)N), ser2(ser);
  bnmf_prune_info a, b;
  std::memset(&a, 0, sizeof a); std::memset(&b, 0, sizeof b);
  prune_finish(members.data(), m, G, N, S, mm.data(), ld.data(), tum.data(), tr.data(), ser.data(), load.data(), tu.data(), sig.data(), &a);
  prune_finish(members.data(), m, G, N, S, mm.data(), ld.data(), tum.data(), tr.data(), ser2.data(), nullptr, nullptr, nullptr, &b);
  if (std::memcmp(&a, &b, sizeof a) != 0 || std::memcmp(ser.data(), ser2.data(), ser.size() * 8) != 0) {
    std::fprintf(stderr, "the info or the series depend on the optional outputs\n"); return 1;
  }
  std::vector<double> out(load);
  out.insert(out.end(), tu.begin(), tu.end());
  out.insert(out.end(), ser.begin(), ser.end());
  out.insert(out.end(), sig.begin(), sig.end());
  for (double v : {(double)a.n_included, (double)a.n_undefined, (double)a.n_single, (double)a.trials, a.max_change}) out.push_back(v);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  std::fwrite(out.data(), 8, out.size(), o);
  std::fclose(o);
  return 0;
}
