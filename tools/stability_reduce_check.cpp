// tools/stability_reduce_check.cpp — bnmf_stability's finish (csrc/reduce_host.h: stability_reduce with con_canon64, and stability_medoid)
// as a stand-alone host program, so that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o stability_reduce_check tools/stability_reduce_check.cpp
//   stability_reduce_check in.bin out.bin
// in.bin: int64 M, N, NPT, K, then off [N + 1] int32, pt [M] int64, D [M][N] and cols [M][K] doubles (the members in the packed order).
// out.bin, all doubles: point [4][NPT], factor [6][N], between [N][N], medoid_at [N], medoid [N][K], then n_points, n_clusters,
// n_negative, mean_silhouette, min_stability, min_stability_at; the same again with every optional output NULL must give the same info
// (checked here).  tests/test_stability_host.py builds it, runs it and holds out.bin to the numpy restatement bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t hd[4];
  if (std::fread(hd, 8, 4, f) != 4 || hd[0] < 2 || hd[1] < 2 || hd[2] < hd[0] || hd[3] < 1) { std::fprintf(stderr, "bad header\n"); return 2; }
  const long M = hd[0], NPT = hd[2]; const int N = (int)hd[1], K = (int)hd[3];
  std::vector<int32_t> off(N + 1); std::vector<int64_t> pt(M); std::vector<double> D((size_t)M * N), cols((size_t)M * K);
  if (std::fread(off.data(), 4, off.size(), f) != off.size() || std::fread(pt.data(), 8, pt.size(), f) != pt.size() ||
      std::fread(D.data(), 8, D.size(), f) != D.size() || std::fread(cols.data(), 8, cols.size(), f) != cols.size()) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);
  std::vector<double> point((size_t)BNMF_STAB_NPOINT * NPT), factor((size_t)BNMF_STAB_NFROW * N), between((size_t)N * N), medoid((size_t)N * K, std::nan(""));
  std::vector<int64_t> at(N), pos(N), pos2(N);
  bnmf_stability_info a, b;
  std::memset(&a, 0, sizeof a); std::memset(&b, 0, sizeof b);
  stability_reduce(D.data(), M, N, off.data(), pt.data(), NPT, point.data(), factor.data(), between.data(), at.data(), pos.data(), &a);
  stability_reduce(D.data(), M, N, off.data(), pt.data(), NPT, nullptr, nullptr, nullptr, nullptr, pos2.data(), &b);
  if (std::memcmp(&a, &b, sizeof a) != 0 || pos != pos2) { std::fprintf(stderr, "the info depends on the optional outputs\n"); return 1; }
  for (int j = 0; j < N; ++j) if (pos[j] >= 0) stability_medoid(cols.data() + (size_t)pos[j] * K, 1, K, medoid.data() + (size_t)j * K);
  std::vector<double> tail;
  for (int j = 0; j < N; ++j) tail.push_back((double)at[j]);
  tail.insert(tail.end(), medoid.begin(), medoid.end());
  for (double v : {(double)a.n_points, (double)a.n_clusters, (double)a.n_negative, a.mean_silhouette, a.min_stability, (double)a.min_stability_at}) tail.push_back(v);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  std::fwrite(point.data(), 8, point.size(), o); std::fwrite(factor.data(), 8, factor.size(), o); std::fwrite(between.data(), 8, between.size(), o);
  std::fwrite(tail.data(), 8, tail.size(), o);
  std::fclose(o);
  return 0;
}
