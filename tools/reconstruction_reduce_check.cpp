// tools/reconstruction_reduce_check.cpp — bnmf_reconstruction's finish (csrc/reduce_host.h: reconstruction_reduce with con_canon64) as a
// stand-alone host program, so that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o reconstruction_reduce_check tools/reconstruction_reduce_check.cpp
//   reconstruction_reduce_check in.bin out.bin
// in.bin: int64 S, N, G, then doubles: min_cosine, tumour [6][G], drop [4][N*G] (each row n + N g), mm [G], ser [S] (the sums over the
// defined tumours).  out.bin, all doubles: series [S], signature [3][N], then n_undefined, n_poor, n_needed, worst_cosine, worst_at; the
// same again with signature NULL must give the same series and info (checked here).  tests/test_reconstruction_host.py builds it, runs it
// and holds out.bin to the numpy restatement bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t hd[3];
  if (std::fread(hd, 8, 3, f) != 3 || hd[0] < 2 || hd[1] < 1 || hd[2] < 1) { std::fprintf(stderr, "bad header\n"); return 2; }
  const int S = (int)hd[0], N = (int)hd[1]; const long G = (long)hd[2];
  const size_t NG = (size_t)N * (size_t)G;
  double min_cosine;
  std::vector<double> tumour((size_t)BNMF_REC_NTUM * G), drop((size_t)BNMF_REC_NDROP * NG), mm(G), ser(S);
  if (std::fread(&min_cosine, 8, 1, f) != 1 || std::fread(tumour.data(), 8, tumour.size(), f) != tumour.size() ||
      std::fread(drop.data(), 8, drop.size(), f) != drop.size() || std::fread(mm.data(), 8, mm.size(), f) != mm.size() ||
      std::fread(ser.data(), 8, ser.size(), f) != ser.size()) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);
  std::vector<double> ser2(ser), sig((size_t)BNMF_REC_NSIG * N);
  bnmf_reconstruction_info a, b;
  std::memset(&a, 0, sizeof a); std::memset(&b, 0, sizeof b);
  reconstruction_reduce(tumour.data(), drop.data(), mm.data(), ser.data(), S, N, G, min_cosine, sig.data(), &a);
  reconstruction_reduce(tumour.data(), drop.data(), mm.data(), ser2.data(), S, N, G, min_cosine, nullptr, &b);
  if (std::memcmp(&a, &b, sizeof a) != 0 || std::memcmp(ser.data(), ser2.data(), ser.size() * 8) != 0) {
    std::fprintf(stderr, "the info or the series depends on the optional output\n");
    return 1;
  }
  std::vector<double> out(ser);
  out.insert(out.end(), sig.begin(), sig.end());
  for (double v : {(double)a.n_undefined, (double)a.n_poor, (double)a.n_needed, a.worst_cosine, (double)a.worst_at}) out.push_back(v);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  std::fwrite(out.data(), 8, out.size(), o);
  std::fclose(o);
  return 0;
}
