// tools/summary_reduce_check.cpp — bnmf_summary's host reduction over the samples (csrc/reduce_host.h: summary_reduce with con_rows,
// con_canon64 and deal_threads) as a stand-alone host program, so that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o summary_reduce_check tools/summary_reduce_check.cpp
//   summary_reduce_check in.bin out.bin
// in.bin: int64 S, int64 N, int64 NSTAT, double ci, then the series [NSTAT][S][N]; out.bin: stat [NSTAT][5][N].
// tests/test_summary_host.py builds it, runs it and holds out.bin to the numpy restatement bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t S = 0, N = 0, Q = 0; double ci = 0.0;
  if (std::fread(&S, 8, 1, f) != 1 || std::fread(&N, 8, 1, f) != 1 || std::fread(&Q, 8, 1, f) != 1 || std::fread(&ci, 8, 1, f) != 1 || S < 1 || N < 1 || Q < 1) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  std::vector<double> ser((size_t)Q * S * N), stat((size_t)Q * BNMF_SUM_NROW * N);
  if (std::fread(ser.data(), 8, ser.size(), f) != ser.size()) { std::fprintf(stderr, "short series\n"); return 2; }
  std::fclose(f);
  summary_reduce(ser.data(), (int)S, (int)N, (int)Q, ci, stat.data());
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  std::fwrite(stat.data(), 8, stat.size(), o);
  std::fclose(o);
  return 0;
}
