// tools/tradeoff_reduce_check.cpp — bnmf_tradeoff's finish (csrc/reduce_host.h: tradeoff_finish with con_canon64) as a stand-alone host
// program, so that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o tradeoff_reduce_check tools/tradeoff_reduce_check.cpp
//   tradeoff_reduce_check in.bin out.bin
// in.bin: int64 m, G, N, C; double min_corr; int32 members [m], pair_at [m], cnts [N*N][3]; doubles tum [3][m], sst [4][C][m], run [N*N][2]
// (what the device leaves: the rows in member order, the pairs' canonB sums and whole-number counts).  out.bin, all doubles: tumour [3][G],
// pair_at [G], pair [5][N*N], setstat [4][C][G], then n_included, n_left_out, n_traded, strongest_pair, strongest_pair_at, mean_ratio; the
// same again with every output NULL must give the same info (checked here).  tests/test_tradeoff_host.py builds it, runs it and holds
// out.bin to the numpy restatement bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t hd[4]; double min_corr;
  if (std::fread(hd, 8, 4, f) != 4 || std::fread(&min_corr, 8, 1, f) != 1 || hd[0] < 1 || hd[1] < hd[0] || hd[2] < 1 || hd[2] > BNMF_TRD_MAX_N || hd[3] < 0 ||
      hd[3] > BNMF_TRD_MAX_C) { std::fprintf(stderr, "bad header\n"); return 2; }
  const long m = (long)hd[0], G = (long)hd[1]; const int N = (int)hd[2], C = (int)hd[3];
  const size_t NN = (size_t)N * N;
  std::vector<int> members(m);
  std::vector<int32_t> pat(m), cnts(NN * 3);
  std::vector<double> tum(3 * (size_t)m), sst((size_t)4 * C * m), run(NN * 2);
  auto get = [&](void* p, size_t size, size_t n) { return n == 0 || std::fread(p, size, n, f) == n; };   // (an empty vector has no address to read to)
  if (!get(members.data(), 4, members.size()) || !get(pat.data(), 4, pat.size()) || !get(cnts.data(), 4, cnts.size()) || !get(tum.data(), 8, tum.size()) ||
      !get(sst.data(), 8, sst.size()) || !get(run.data(), 8, run.size())) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);
  for (long i = 0; i < m; ++i)
    if (members[i] < 0 || members[i] >= G || (i && members[i] <= members[i - 1])) { std::fprintf(stderr, "bad member list\n"); return 2; }
  std::vector<double> tu(3 * (size_t)G), pr(5 * NN), ss((size_t)4 * C * G);
  std::vector<int32_t> pa(G);
  bnmf_tradeoff_info a, b;
  std::memset(&a, 0, sizeof a); std::memset(&b, 0, sizeof b);
  tradeoff_finish(members.data(), m, G, N, C, min_corr, tum.data(), pat.data(), sst.data(), run.data(), cnts.data(), tu.data(), pa.data(), pr.data(),
                  C ? ss.data() : nullptr, &a);
  tradeoff_finish(members.data(), m, G, N, C, min_corr, tum.data(), pat.data(), sst.data(), run.data(), cnts.data(), nullptr, nullptr, nullptr, nullptr, &b);
  if (std::memcmp(&a, &b, sizeof a) != 0) { std::fprintf(stderr, "the info depends on the optional outputs\n"); return 1; }
  std::vector<double> out(tu);
  out.insert(out.end(), pa.begin(), pa.end());
  out.insert(out.end(), pr.begin(), pr.end());
  out.insert(out.end(), ss.begin(), ss.end());
  for (double v : {(double)a.n_included, (double)a.n_left_out, (double)a.n_traded, a.strongest_pair, (double)a.strongest_pair_at, a.mean_ratio}) out.push_back(v);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  std::fwrite(out.data(), 8, out.size(), o);
  std::fclose(o);
  return 0;
}
