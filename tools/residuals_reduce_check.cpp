// tools/residuals_reduce_check.cpp — bnmf_residuals' host side (csrc/reduce_host.h: residuals_lead and residuals_finish with con_rows and
// con_canon64) as a stand-alone host program, so that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o residuals_reduce_check tools/residuals_reduce_check.cpp
//   residuals_reduce_check in.bin out.bin
// in.bin: int64 m, G, K, S, n_steps; double max_dispersion; int32 members [m]; doubles C [S][K][K] (each symmetric), b [S][K],
// z [S][K][m] (made-up residuals in member order).  What the device leaves per sample is formed here by the host's own routine: the
// component, the series and flat by residuals_lead, the scores and chi from z in the spec's order, the mean matrix by con_canon64 over
// the samples that are not flat.  out.bin, all doubles: flat [S], gram [K*K], type [5][K], component [4][K], tumour [3][G], series
// [5][S], then n_flat, n_included, n_left_out, n_biased, n_overdispersed, worst_type_at, min_agreement_at, lambda, share, move,
// mean_share, min_agreement, worst_type; the same again with every output NULL must give the same info (checked here).
// tests/test_residuals_host.py builds it, runs it and holds out.bin to the numpy restatement bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t hd[5]; double max_dispersion;
  if (std::fread(hd, 8, 5, f) != 5 || std::fread(&max_dispersion, 8, 1, f) != 1 || hd[0] < 2 || hd[1] < hd[0] || hd[2] < 1 || hd[2] > BNMF_RES_MAX_K || hd[3] < 2 ||
      hd[4] < 1 || hd[4] > BNMF_RES_MAX_STEPS) { std::fprintf(stderr, "bad header\n"); return 2; }
  const long m = (long)hd[0], G = (long)hd[1]; const int K = (int)hd[2], S = (int)hd[3], n_steps = (int)hd[4];
  const size_t KK = (size_t)K * K;
  std::vector<int> members(m);
  std::vector<double> C((size_t)S * KK), b((size_t)S * K), z((size_t)S * K * m);
  if (std::fread(members.data(), 4, members.size(), f) != members.size() || std::fread(C.data(), 8, C.size(), f) != C.size() ||
      std::fread(b.data(), 8, b.size(), f) != b.size() || std::fread(z.data(), 8, z.size(), f) != z.size()) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);
  for (long i = 0; i < m; ++i)
    if (members[i] < 0 || members[i] >= G || (i && members[i] <= members[i - 1])) { std::fprintf(stderr, "bad member list\n"); return 2; }
  // what the device leaves per sample
  std::vector<int32_t> flat(S);
  std::vector<double> v((size_t)S * K), q((size_t)S * K), ser4(4 * (size_t)S), t((size_t)S * m), chi((size_t)S * m), y(K), gram(KK), col;
  int Sp = 0;
  for (int s = 0; s < S; ++s) {
    res_lead ld;
    const bool ok = residuals_lead(C.data() + (size_t)s * KK, K, n_steps, v.data() + (size_t)s * K, y.data(), &ld);
    flat[s] = ok ? 0 : 1; Sp += ok ? 1 : 0;
    ser4[s] = ld.trace; ser4[(size_t)S + s] = ld.lambda; ser4[2 * (size_t)S + s] = ld.share; ser4[3 * (size_t)S + s] = ld.move;
    for (int k = 0; k < K; ++k) q[(size_t)s * K + k] = C[(size_t)s * KK + (size_t)k * K + k];
    const double* zs = z.data() + (size_t)s * K * m;
    for (long i = 0; i < m; ++i) {
      double ts = 0.0, cs = 0.0;
      for (int k = 0; k < K; ++k) { const double zz = zs[(size_t)k * m + i]; ts = ts + v[(size_t)s * K + k] * zz; cs = cs + zz * zz; }
      t[(size_t)s * m + i] = ts; chi[(size_t)s * m + i] = cs / (double)K;
    }
  }
  if (Sp < 2) { std::fprintf(stderr, "fewer than 2 samples that are not flat\n"); return 2; }
  for (size_t e = 0; e < KK; ++e) {
    col.clear();
    for (int s = 0; s < S; ++s) if (!flat[s]) col.push_back(C[(size_t)s * KK + e]);
    gram[e] = con_canon64(col.data(), col.size(), 1) / (double)Sp;
  }
  std::vector<double> type((size_t)BNMF_RES_NTYPE * K), comp((size_t)BNMF_RES_NCOMP * K), tum((size_t)BNMF_RES_NTUM * G), series((size_t)BNMF_RES_NSER * S);
  bnmf_residuals_info info, bare;
  std::memset(&info, 0, sizeof info); std::memset(&bare, 0, sizeof bare);
  residuals_finish(members.data(), m, G, K, S, n_steps, max_dispersion, flat.data(), gram.data(), ser4.data(), b.data(), q.data(), v.data(), t.data(), chi.data(),
                   type.data(), comp.data(), tum.data(), series.data(), &info);
  residuals_finish(members.data(), m, G, K, S, n_steps, max_dispersion, flat.data(), gram.data(), ser4.data(), b.data(), q.data(), v.data(), t.data(), chi.data(),
                   nullptr, nullptr, nullptr, nullptr, &bare);
  if (std::memcmp(&info, &bare, sizeof info) != 0) { std::fprintf(stderr, "the info fields depend on the outputs asked for\n"); return 1; }
  f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  std::vector<double> fl(flat.begin(), flat.end());
  const double tail[13] = {(double)info.n_flat, (double)info.n_included, (double)info.n_left_out, (double)info.n_biased, (double)info.n_overdispersed,
                           (double)info.worst_type_at, (double)info.min_agreement_at, info.lambda, info.share, info.move, info.mean_share, info.min_agreement,
                           info.worst_type};
  bool ok = std::fwrite(fl.data(), 8, fl.size(), f) == fl.size() && std::fwrite(gram.data(), 8, gram.size(), f) == gram.size() &&
            std::fwrite(type.data(), 8, type.size(), f) == type.size() && std::fwrite(comp.data(), 8, comp.size(), f) == comp.size() &&
            std::fwrite(tum.data(), 8, tum.size(), f) == tum.size() && std::fwrite(series.data(), 8, series.size(), f) == series.size() &&
            std::fwrite(tail, 8, 13, f) == 13;
  ok = std::fclose(f) == 0 && ok;
  return ok ? 0 : 2;
}
