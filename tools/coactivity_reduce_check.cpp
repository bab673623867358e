// tools/coactivity_reduce_check.cpp — bnmf_coactivity's host reduction over the samples (csrc/reduce_host.h: coactivity_reduce with
// con_rows, con_canon64 and deal_threads) as a stand-alone host program, so that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o coactivity_reduce_check tools/coactivity_reduce_check.cpp
//   coactivity_reduce_check in.bin out.bin
// in.bin: int64 S, int64 NP, double ci, then the series [4][S][NP]; out.bin: pair [4][7][NP], then n_credible[3], max_cosine_at and
// max_cosine as doubles; the same again with pair = NULL must give the same counts (checked here).  tests/test_coactivity_host.py builds
// it, runs it and holds out.bin to the numpy restatement bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t S = 0, NP = 0; double ci = 0.0;
  if (std::fread(&S, 8, 1, f) != 1 || std::fread(&NP, 8, 1, f) != 1 || std::fread(&ci, 8, 1, f) != 1 || S < 1 || NP < 1) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<double> ser((size_t)BNMF_COA_NSTAT * S * NP), pair((size_t)BNMF_COA_NSTAT * BNMF_COA_NPROW * NP);
  if (std::fread(ser.data(), 8, ser.size(), f) != ser.size()) { std::fprintf(stderr, "short series\n"); return 2; }
  std::fclose(f);
  int64_t nc[3], at = 0, nc2[3], at2 = 0; double mx = 0.0, mx2 = 0.0;
  coactivity_reduce(ser.data(), (int)S, (long)NP, ci, pair.data(), nc, &at, &mx);
  coactivity_reduce(ser.data(), (int)S, (long)NP, ci, nullptr, nc2, &at2, &mx2);
  if (nc[0] != nc2[0] || nc[1] != nc2[1] || nc[2] != nc2[2] || at != at2 || std::memcmp(&mx, &mx2, 8) != 0) { std::fprintf(stderr, "the counts depend on pair\n"); return 1; }
  const double tail[5] = {(double)nc[0], (double)nc[1], (double)nc[2], (double)at, mx};
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  std::fwrite(pair.data(), 8, pair.size(), o);
  std::fwrite(tail, 8, 5, o);
  std::fclose(o);
  return 0;
}
