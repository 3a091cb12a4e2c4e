// The gain-tuning GA of the reference (GA/pdGA.py) as a device step: a counter-based random stream and one
// generation's breeding -- rewards and running averages (GA/mpcGA.py:40-56), roulette selection (pdGA.py:57-62),
// one-point crossover (:64-69), mutation (:71-76), replacement of the lowest rewards (:87) -- one 64-lane
// wavefront per island, fp64, host + gfx950.  The genes are opaque doubles: the PID gains of mpcracing/pid.py
// or the runtime parameters of mpcracing/ga.py.
#pragma once
#include "mr_wave_prims.h"

namespace mr {

#define MR_GA_P_MAX 64
#define MR_GA_K_MAX 64
#define MR_GA_D_MAX 16

// ---- the random stream: Philox4x64-10 as numpy.random.Philox defines it ----
MR_HD void ga_mul64(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  hi = __umul64hi(a, b);
#else
  hi = (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
  lo = a * b;
}
// out = philox4x64-10(ctr, key)
MR_HD void ga_philox(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1, uint64_t* out) {
  for (int r = 0; r < 10; ++r) {
    uint64_t h0, l0, h1, l1;
    ga_mul64(0xD2E7470EE14C6C93ull, c0, h0, l0);
    ga_mul64(0xCA5A826395121157ull, c2, h1, l1);
    const uint64_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B97F4A7C15ull;
    k1 += 0xBB67AE8584CAA73Bull;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// Raw draw j of the stream (seed, island, generation) =
// numpy.random.Philox(key=[seed, island], counter=[0, 0, generation, 0]).random_raw()[j]: numpy increments the
// counter before its first block, so draw j is word j % 4 of the block at counter [j / 4 + 1, 0, generation, 0].
struct GaStream {
  uint64_t seed, island, generation;
  uint64_t block;  // the block held in w (0: none)
  uint64_t w0, w1, w2, w3;
  MR_HD GaStream(uint64_t s, uint64_t i, uint64_t g) : seed(s), island(i), generation(g), block(0), w0(0), w1(0), w2(0), w3(0) {}
  MR_HD uint64_t raw(uint64_t j) {
    const uint64_t b = j / 4 + 1;
    if (b != block) {
      uint64_t o[4];
      ga_philox(b, 0, generation, 0, seed, island, o);
      w0 = o[0]; w1 = o[1]; w2 = o[2]; w3 = o[3];
      block = b;
    }
    const int q = (int)(j & 3);
    return q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : w3;
  }
  // numpy.random.Generator.random(): (raw >> 11) * 2^-53, in [0, 1)
  MR_HD double u01(uint64_t j) { return (double)(raw(j) >> 11) * (1.0 / 9007199254740992.0); }
};

struct GaBreedArgs {
  int n_island, P, K, D, pairs;
  double kT, lambda_T, mutation_rate;
  uint64_t seed, island0, generation;
  double* genes;        // gene d of individual i of island j at genes[(j P + i) ld + col[d]], in/out
  int ld;               // row stride in doubles
  int col[MR_GA_D_MAX]; // the genes' columns in a row (distinct, in [0, ld))
  const double* times;  // [n_island][P][K], inf = not finished
  double* avg;          // [n_island][K] in/out
  const double* lo;     // [D] or null; NaN = no bound
  const double* hi;     // [D] or null
  double* r;            // [n_island][P]
  double* best_r;       // [n_island]
  int32_t* best_idx;    // [n_island]
  double* best_genes;   // [n_island][D], as they were before the replacement
};
// col null: gene d is column d
inline GaBreedArgs make_ga_breed_args(int n_island, int P, int K, int D, int pairs, double* genes, int ld,
                                      const int32_t* col, const double* times, double* avg, const double* lo,
                                      const double* hi, double kT, double lambda_T, double mutation_rate,
                                      uint64_t seed, uint64_t island0, uint64_t generation, double* r, double* best_r,
                                      int32_t* best_idx, double* best_genes) {
  GaBreedArgs A{n_island, P, K, D, pairs, kT, lambda_T, mutation_rate, seed, island0, generation, genes, ld, {},
                times, avg, lo, hi, r, best_r, best_idx, best_genes};
  for (int d = 0; d < MR_GA_D_MAX; ++d) A.col[d] = col && d < D ? col[d] : d;
  return A;
}

inline const char* ga_breed_check(int64_t n_island, int64_t P, int64_t K, int64_t D, int64_t pairs, int64_t ld,
                                  const int32_t* col, double kT, double lambda_T, double mutation_rate) {
  if (n_island < 0) return "n_island < 0";
  if (P < 2 || P > MR_GA_P_MAX) return "P outside 2..64";
  if (K < 1 || K > MR_GA_K_MAX) return "K outside 1..64";
  if (D < 1 || D > MR_GA_D_MAX) return "D outside 1..16";
  if (pairs < 1) return "pairs < 1";
  if (2 * pairs > P) return "2 pairs > P (every child replaces another individual)";
  if (col) {
    for (int d = 0; d < D; ++d) {
      if (col[d] < 0 || col[d] >= ld) return "col entry outside [0, ld)";
      for (int e = 0; e < d; ++e)
        if (col[e] == col[d]) return "col entries must be distinct";
    }
  } else if (ld < D) {
    return "ld < D";
  }
  if (n_island * P * ld > (int64_t)0x7fffffff) return "too many genes";
  if (!(kT == kT) || !(lambda_T == lambda_T) || !(mutation_rate == mutation_rate)) return "kT, lambda_T or mutation_rate is NaN";
  return nullptr;
}

MR_HD bool ga_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
// np.argsort(r, kind="stable") order: (r[j], j) before (r[i], i); a NaN sorts last
MR_HD bool ga_before(double rj, int j, double ri, int i) {
  const bool nj = rj != rj, ni = ri != ri;
  if (ni) return !nj || j < i;
  return !nj && (rj < ri || (rj == ri && j < i));
}

// The shared memory of one island's wavefront (LDS on the device)
constexpr int GA_LDC = MR_GA_K_MAX + 1;  // padded row of the contributions: lane i reads row i
struct GaShared {
  double contrib[MR_GA_P_MAX * GA_LDC];  // exp(-kT (t - a)) of (i, k), 0 where unfinished
  double r[MR_GA_P_MAX];
  double cdf[MR_GA_P_MAX];
  double child[MR_GA_P_MAX * MR_GA_D_MAX];
  int slot[MR_GA_P_MAX];  // slot[q]: the individual with the q-th lowest reward
  int best;
};

// One generation of island `isl` of the call.  Every lane reaches every wsync.
#if MR_DEVICE_BUILD
__device__ __forceinline__
#else
inline
#endif
void ga_breed_island(const Wv& w, const GaBreedArgs& A, int isl, GaShared* sh) {
  const int l = w.lane, P = A.P, K = A.K, D = A.D;
  const int ld = A.ld;
  double* genes = A.genes + (int64_t)isl * P * ld;
  const double* times = A.times + (int64_t)isl * P * K;
  double* avg = A.avg + (int64_t)isl * K;
  // 1. rewards and averages: lane k runs segment k over the individuals in order
  if (l < K) {
    double a = avg[l];
    for (int i = 0; i < P; ++i) {
      const double t = times[(int64_t)i * K + l];
      double c = 0.0;
      if (ga_finite(t)) {
        c = exp(-A.kT * (t - a));
        a = A.lambda_T * t + (1 - A.lambda_T) * a;
      }
      sh->contrib[i * GA_LDC + l] = c;
    }
    avg[l] = a;
  }
  wsync(w);
  if (l < P) {
    double r = 0.0;
    for (int k = 0; k < K; ++k) r += sh->contrib[l * GA_LDC + k];
    sh->r[l] = r;
    A.r[(int64_t)isl * P + l] = r;
  }
  wsync(w);
  // 2. the cumulative sum in index order, each individual's place in the stable ascending order, the best
  if (l == 0) {
    double c = 0.0;
    for (int i = 0; i < P; ++i) {
      c += sh->r[i];
      sh->cdf[i] = c;
    }
  }
  if (l < P) {
    const double ri = sh->r[l];
    int below = 0, better = 0;
    for (int j = 0; j < P; ++j) {
      const double rj = sh->r[j];
      below += (j != l && ga_before(rj, j, ri, l)) ? 1 : 0;
      // np.argmax: the first maximum, the first NaN if there is one
      const bool nj = rj != rj, ni = ri != ri;
      better += (j != l && (rj > ri || (rj == ri && j < l) || (nj && (!ni || j < l)))) ? 1 : 0;
    }
    sh->slot[below] = l;
    if (better == 0) sh->best = l;
  }
  wsync(w);
  // 3. lane q builds child q % 2 of pair q / 2 from the population as it is
  const int n_child = 2 * A.pairs;
  if (l < n_child) {
    const int m = l >> 1, c = l & 1;
    GaStream rs(A.seed, A.island0 + (uint64_t)isl, A.generation);
    const uint64_t base = (uint64_t)m * (uint64_t)(3 + 4 * D);
    const double total = sh->cdf[P - 1];
    int par[2];
    for (int s = 0; s < 2; ++s) {
      const double u = rs.u01(base + s);
      int j;
      if (total == 0.0 || !ga_finite(total)) {
        j = (int)floor(u * P);
        j = j > P - 1 ? P - 1 : j;
      } else {
        const double x = u * total;
        j = P - 1;
        for (int q = P - 1; q >= 0; --q) j = x < sh->cdf[q] ? q : j;  // the first q with x < cdf[q]
      }
      par[s] = j;
    }
    const int pt = 1 + (int)floor(rs.u01(base + 2) * (D - 1));
    const double* ga = genes + (int64_t)par[c] * ld;      // child 0 = a[:pt] ++ b[pt:], child 1 = b[:pt] ++ a[pt:]
    const double* gb = genes + (int64_t)par[1 - c] * ld;
    const uint64_t fl = base + 3 + (uint64_t)c * (uint64_t)(2 * D);
    for (int d = 0; d < D; ++d) sh->child[l * MR_GA_D_MAX + d] = rs.u01(fl + d);  // the flags, in draw order
    for (int d = 0; d < D; ++d) {
      double g = d < pt ? ga[A.col[d]] : gb[A.col[d]];
      const double flag = sh->child[l * MR_GA_D_MAX + d];
      const double v = rs.u01(fl + D + d);
      if (flag < A.mutation_rate) g += v - 0.5;
      if (A.lo) {
        const double b = A.lo[d];
        if (b == b && g < b) g = b;
      }
      if (A.hi) {
        const double b = A.hi[d];
        if (b == b && g > b) g = b;
      }
      sh->child[l * MR_GA_D_MAX + d] = g;
    }
  }
  // 5. the best individual as it was before the replacement
  const int best = sh->best;
  if (l < D) A.best_genes[(int64_t)isl * D + l] = genes[(int64_t)best * ld + A.col[l]];
  if (l == 0) {
    A.best_r[isl] = sh->r[best];
    A.best_idx[isl] = best;
  }
  wsync(w);
  // 4. the 2 pairs lowest rewards take the children in order
  if (l < n_child) {
    double* dst = genes + (int64_t)sh->slot[l] * ld;
    for (int d = 0; d < D; ++d) dst[A.col[d]] = sh->child[l * MR_GA_D_MAX + d];
  }
}

}  // namespace mr
