// Sanchez-Garcia multiple-linear-regression band ratio (starcop/data/feature_extration.py:58-125).
// Per tile: least squares of the target band on k regressor bands with an intercept (sklearn LinearRegression over all
// pixels, zeros included), the prediction r, then one of three divisions of the target by r.
//   moments : one pass over the k+1 planes, fp32 16-byte loads, fp64 sums of z and of the upper triangle of z z^T
//             (z = [x_1..x_k, t] minus a per-band shift = the tile's centre pixel); per-work-group partials, no atomics
//   solve   : one wave per tile; partials summed in a fixed order, centred Gram, unit-diagonal equilibration, cyclic
//             Jacobi eigen-solve in fp64, minimum-norm solution (eigenvalues below 1e-12 * max dropped, zero-variance
//             columns get coefficient 0) -> coef[B][k+1], intercept last
//   predict : r = intercept + sum_j coef_j x_j in fp64, stored fp32 (c_matched_outliers); the other divisions evaluate r
//             in fp64 inside their own passes
//   ratio   : c_matched_outliers (sc_trimmed_sums of t and r, then the sc_band_ratio arithmetic with background t and
//             signal r), simple_plus (fp64 mean / std / min of R0 = -t/(r+1e-6), then one elementwise pass) or residual
#include "sc_common.h"

namespace {

constexpr int KMAX = 9;
constexpr int NM_MAX = (KMAX + 1) + (KMAX + 1) * (KMAX + 2) / 2;     // 65 moments at k = 9

struct MlrD {
  const float* base;
  long long off[16];
  long long ts;
  const float* tgt;
  long long tts;
  size_t n;
  int k;
};

__device__ __forceinline__ const float* mlr_plane(const MlrD& a, int tile, int j) {
  return j < a.k ? a.base + (long long)tile * a.ts + a.off[j] : a.tgt + (long long)tile * a.tts;
}

// work-groups per tile of the streaming kernels: a function of n only, so a tile's sums do not depend on the batch around it
inline unsigned mlr_groups(size_t n) {
  const size_t g = (n + 4095) / 4096;
  return (unsigned)(g < 1 ? 1 : (g > 64 ? 64 : g));
}
constexpr int nmom(int k) { return (k + 1) + (k + 1) * (k + 2) / 2; }

template <int D>
__device__ __forceinline__ void mlr_accum(double* acc, const double* z) {
#pragma unroll
  for (int a = 0; a < D; ++a) acc[a] += z[a];
  int m = D;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b, ++m) acc[m] = fma(z[a], z[b], acc[m]);
}

// part[tile][blockIdx.x][NM]: [sum z_a (a < D)] then [sum z_a z_b (a <= b, row-major upper triangle)]
template <int K>
__global__ __launch_bounds__(256) void k_mlr_moments(MlrD a, int vec, double* __restrict__ part) {
  constexpr int D = K + 1, NM = nmom(K);
  __shared__ double red[4][NM];
  const int tile = blockIdx.y;
  const unsigned G = gridDim.x;
  const float* p[D];
  double s[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    p[j] = mlr_plane(a, tile, j);
    s[j] = (double)p[j][a.n / 2];
  }
  double acc[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) acc[m] = 0.0;
  size_t i0 = 0;
  if (vec) {
    const size_t n4 = a.n >> 2;
    for (size_t q = blockIdx.x * (size_t)256 + threadIdx.x; q < n4; q += (size_t)G * 256) {
      float4 v[D];
#pragma unroll
      for (int j = 0; j < D; ++j) v[j] = reinterpret_cast<const float4*>(p[j])[q];
      double z[D];
#pragma unroll
      for (int j = 0; j < D; ++j) z[j] = (double)v[j].x - s[j];
      mlr_accum<D>(acc, z);
#pragma unroll
      for (int j = 0; j < D; ++j) z[j] = (double)v[j].y - s[j];
      mlr_accum<D>(acc, z);
#pragma unroll
      for (int j = 0; j < D; ++j) z[j] = (double)v[j].z - s[j];
      mlr_accum<D>(acc, z);
#pragma unroll
      for (int j = 0; j < D; ++j) z[j] = (double)v[j].w - s[j];
      mlr_accum<D>(acc, z);
    }
    i0 = n4 << 2;
  }
  for (size_t i = i0 + blockIdx.x * (size_t)256 + threadIdx.x; i < a.n; i += (size_t)G * 256) {
    double z[D];
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = (double)p[j][i] - s[j];
    mlr_accum<D>(acc, z);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const double v = wave_sum_d(acc[m]);
    if (lane == 0) red[w][m] = v;
  }
  __syncthreads();
  for (int m = threadIdx.x; m < NM; m += 256)
    part[((size_t)tile * G + blockIdx.x) * NM + m] = ((red[0][m] + red[1][m]) + red[2][m]) + red[3][m];
}

// packed index of (a, b), a <= b, in the moment row
__device__ __forceinline__ int tri(int D, int a, int b) {
  if (a > b) { const int t = a; a = b; b = t; }
  return D + a * D - a * (a - 1) / 2 + (b - a);
}

__global__ __launch_bounds__(64) void k_mlr_solve(MlrD a, const double* __restrict__ part, int G, double* __restrict__ coef) {
  __shared__ double mom[NM_MAX];
  __shared__ double A[KMAX][KMAX], V[KMAX][KMAX], g[KMAX], dsc[KMAX];
  __shared__ int act[KMAX];
  const int tile = blockIdx.x, lane = threadIdx.x, K = a.k, D = K + 1, NM = nmom(K);
  for (int m = lane; m < NM; m += 64) {
    double v = 0.0;
    for (int q = 0; q < G; ++q) v += part[((size_t)tile * G + q) * NM + m];
    mom[m] = v;
  }
  __syncthreads();
  const double n = (double)a.n;
  if (lane == 0) {
    for (int i = 0; i < K; ++i) {
      const double raw = mom[tri(D, i, i)];
      const double cii = raw - mom[i] * mom[i] / n;
      act[i] = cii > 0.0 && cii > 1e-13 * raw;
      dsc[i] = act[i] ? sqrt(cii) : 1.0;
    }
    for (int i = 0; i < K; ++i) {
      for (int j = 0; j < K; ++j) {
        const double cij = mom[tri(D, i, j)] - mom[i] * mom[j] / n;
        A[i][j] = (act[i] && act[j]) ? (i == j ? 1.0 : cij / (dsc[i] * dsc[j])) : 0.0;
        V[i][j] = i == j ? 1.0 : 0.0;
      }
      g[i] = act[i] ? (mom[tri(D, i, K)] - mom[i] * mom[K] / n) / dsc[i] : 0.0;
    }
  }
  __syncthreads();
  // cyclic Jacobi: A <- J^T A J, V <- V J, one (p, q) rotation at a time; lane j owns row j (column pass) and column j (row pass)
  for (int sweep = 0; sweep < 50; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < K; ++i) {
      dia += A[i][i] * A[i][i];
      for (int j = i + 1; j < K; ++j) off += A[i][j] * A[i][j];
    }
    if (off <= 1e-30 * dia) break;
    for (int p = 0; p < K - 1; ++p) {
      for (int q = p + 1; q < K; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        __syncthreads();
        if (lane < K) {
          const double ap = A[lane][p], aq = A[lane][q];
          A[lane][p] = c * ap - s * aq; A[lane][q] = s * ap + c * aq;
          const double vp = V[lane][p], vq = V[lane][q];
          V[lane][p] = c * vp - s * vq; V[lane][q] = s * vp + c * vq;
        }
        __syncthreads();
        if (lane < K) {
          const double ap = A[p][lane], aq = A[q][lane];
          A[p][lane] = c * ap - s * aq; A[q][lane] = s * ap + c * aq;
        }
        __syncthreads();
      }
    }
  }
  if (lane == 0) {
    double lmax = 0.0;
    for (int e = 0; e < K; ++e) lmax = fmax(lmax, A[e][e]);
    double y[KMAX];
    for (int i = 0; i < K; ++i) y[i] = 0.0;
    for (int e = 0; e < K; ++e) {
      const double lam = A[e][e];
      if (!(lam > 1e-12 * lmax)) continue;
      double proj = 0.0;
      for (int l = 0; l < K; ++l) proj += V[l][e] * g[l];
      proj /= lam;
      for (int i = 0; i < K; ++i) y[i] += V[i][e] * proj;
    }
    // means of the unshifted bands: shift + shifted sum / n
    const double mean_t = (double)mlr_plane(a, tile, K)[a.n / 2] + mom[K] / n;
    double icpt = mean_t;
    for (int i = 0; i < K; ++i) {
      const double ci = act[i] ? y[i] / dsc[i] : 0.0;
      coef[(size_t)tile * D + i] = ci;
      icpt -= ci * ((double)mlr_plane(a, tile, i)[a.n / 2] + mom[i] / n);
    }
    coef[(size_t)tile * D + K] = icpt;
  }
}

// the regressor planes and coefficients of one tile, for the kernels that evaluate r = intercept + sum_j coef_j x_j
template <int K>
struct MlrTile {
  const float* p[K];
  double c[K + 1];
  __device__ __forceinline__ MlrTile(const MlrD& a, const double* coef, int tile) {
#pragma unroll
    for (int j = 0; j < K; ++j) p[j] = mlr_plane(a, tile, j);
#pragma unroll
    for (int j = 0; j <= K; ++j) c[j] = coef[(size_t)tile * (K + 1) + j];
  }
  __device__ __forceinline__ double r64(size_t i) const {
    double v = c[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v = fma(c[j], (double)p[j][i], v);
    return v;
  }
};

template <int K>
__global__ __launch_bounds__(256) void k_mlr_predict(MlrD a, const double* __restrict__ coef, float* __restrict__ r) {
  const int tile = blockIdx.y;
  const MlrTile<K> m(a, coef, tile);
  float* rt = r + (size_t)tile * a.n;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < a.n; i += (size_t)gridDim.x * 256) rt[i] = (float)m.r64(i);
}

// simple_plus statistics of R0 = -t/(r+1e-6), r in fp64: part[tile][blockIdx.x] = {sum, sum of squares, min}
template <int K>
__global__ __launch_bounds__(256) void k_mlr_sp_stats(MlrD a, const double* __restrict__ coef, double* __restrict__ part) {
  __shared__ double red[4][3];
  const int tile = blockIdx.y;
  const MlrTile<K> m(a, coef, tile);
  const float* t = mlr_plane(a, tile, a.k);
  double s1 = 0.0, s2 = 0.0, mn = __builtin_inf();
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < a.n; i += (size_t)gridDim.x * 256) {
    const double v = -(double)t[i] / (m.r64(i) + 1e-6);
    s1 += v; s2 = fma(v, v, s2); mn = fmin(mn, v);
  }
  s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { red[w][0] = s1; red[w][1] = s2; red[w][2] = mn; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    const double v = q == 2 ? fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]))
                            : ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    part[((size_t)tile * gridDim.x + blockIdx.x) * 3 + q] = v;
  }
}

__device__ __forceinline__ float mlr_clip(float v, int autoclip) {
  return autoclip ? (v < -0.2f ? -0.2f : (v > 0.2f ? 0.2f : v)) : v;       // np.clip: NaN stays NaN
}

// c_matched_outliers divides by the stored fp32 r (its trimmed sums are taken on r); simple_plus and residual evaluate r in
// fp64 in place, so the only rounding of their result is the final one
template <int K>
__global__ __launch_bounds__(256) void k_mlr_ratio(MlrD a, const double* __restrict__ coef, const float* __restrict__ r, int division,
                                                   const double* __restrict__ sums, const double* __restrict__ sp_part, int G,
                                                   int autoclip, float* __restrict__ out) {
  __shared__ double s_mean, s_std, s_min;
  const int tile = blockIdx.y;
  const float* t = mlr_plane(a, tile, a.k);
  float* ot = out + (size_t)tile * a.n;
  const size_t step = (size_t)gridDim.x * 256;
  if (division == SC_MLR_C_MATCHED) {
    const float* rt = r + (size_t)tile * a.n;
    const float c = (float)sums[tile] / (float)sums[gridDim.y + tile];       // float32 division, as sc_band_ratio
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < a.n; i += step) {
      const float b = t[i], s = rt[i];
      const float v = (c * s - b) / (b + 1e-6f);
      ot[i] = mlr_clip(((s < 1e-6f && b < 1e-6f) || b == 0.f) ? -0.5f : v, autoclip);
    }
    return;
  }
  const MlrTile<K> m(a, coef, tile);
  if (division == SC_MLR_RESIDUAL) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < a.n; i += step) {
      const float b = t[i];
      const double rv = m.r64(i);
      ot[i] = mlr_clip(b == 0.f ? 0.f : (float)(((double)b - rv) / (rv + 1e-6)), autoclip);
    }
    return;
  }
  if (threadIdx.x == 0) {            // every work-group of the tile sums the partials in the same order
    double s1 = 0.0, s2 = 0.0, mn = __builtin_inf();
    for (int q = 0; q < G; ++q) {
      const double* pp = sp_part + ((size_t)tile * G + q) * 3;
      s1 += pp[0]; s2 += pp[1]; mn = fmin(mn, pp[2]);
    }
    const double n = (double)a.n, mean = s1 / n;
    double var = s2 / n - mean * mean;
    if (var < 0.0) var = 0.0;
    s_mean = mean; s_std = sqrt(var); s_min = mn;
  }
  __syncthreads();
  const double mean = s_mean, sd = s_std;
  const float rmin = (float)((s_min - mean) / sd);          // min(R) = (min(R0) - mean) / std
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < a.n; i += step) {
    const float b = t[i];
    const float v = (float)((-(double)b / (m.r64(i) + 1e-6) - mean) / sd);
    ot[i] = mlr_clip(b == 0.f ? rmin : v, autoclip);
  }
}

MlrD to_mlrd(const sc_mlr_args& s) {
  MlrD d;
  d.base = s.base;
  for (int j = 0; j < 16; ++j) d.off[j] = s.band_off[j];
  d.ts = s.tile_stride; d.tgt = s.target; d.tts = s.target_tile_stride; d.n = s.n; d.k = s.k;
  return d;
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

struct MlrWork {
  double* part;      // [B][G][NM_MAX] moment partials
  double* sp;        // [B][G][3] simple_plus partials
  double* sums;      // [2][B] trimmed sums of t and r
  void* trim;        // sc_trimmed_sums workspace
  float* tcopy;      // [B][n] dense copy of a strided target for sc_trimmed_sums
  size_t trim_bytes;
};

MlrWork carve(void* work, int B, size_t n) {
  const size_t G = mlr_groups(n);
  char* p = reinterpret_cast<char*>(work);
  MlrWork w;
  w.part = reinterpret_cast<double*>(p); p += al256((size_t)B * G * NM_MAX * sizeof(double));
  w.sp = reinterpret_cast<double*>(p); p += al256((size_t)B * G * 3 * sizeof(double));
  w.sums = reinterpret_cast<double*>(p); p += al256((size_t)2 * B * sizeof(double));
  w.trim_bytes = sc_trimmed_sum_workspace_bytes(B);
  w.trim = p; p += al256(w.trim_bytes);
  w.tcopy = reinterpret_cast<float*>(p);
  return w;
}

int check_args(const sc_mlr_args* a, const char* name) {
  SC_REQUIRE(a && a->base && a->target, "%s: bad argument", name);
  SC_REQUIRE(a->k >= 1 && a->k <= KMAX, "%s: k = %d regressors (1..%d supported)", name, a->k, KMAX);
  SC_REQUIRE(a->B >= 1 && a->B <= 65535 && a->n >= 2, "%s: bad shape (B %d, n %zu)", name, a->B, a->n);
  return SC_OK;
}

template <int K>
void launch_moments(const MlrD& d, int B, int vec, double* part, hipStream_t st) {
  hipLaunchKernelGGL(k_mlr_moments<K>, dim3(mlr_groups(d.n), B), dim3(256), 0, st, d, vec, part);
}
template <int K>
void launch_sp_stats(const MlrD& d, int B, const double* coef, double* part, hipStream_t st) {
  hipLaunchKernelGGL(k_mlr_sp_stats<K>, dim3(mlr_groups(d.n), B), dim3(256), 0, st, d, coef, part);
}
template <int K>
void launch_ratio(const MlrD& d, int B, const double* coef, const float* r, int division, const double* sums, const double* sp,
                  int autoclip, float* out, hipStream_t st) {
  const unsigned bx = (unsigned)((d.n + 2047) / 2048 > 256 ? 256 : (d.n + 2047) / 2048);
  hipLaunchKernelGGL(k_mlr_ratio<K>, dim3(bx, B), dim3(256), 0, st, d, coef, r, division, sums, sp, (int)mlr_groups(d.n), autoclip, out);
}
template <int K>
void launch_predict(const MlrD& d, int B, const double* coef, float* r, hipStream_t st) {
  const unsigned bx = (unsigned)((d.n + 2047) / 2048 > 256 ? 256 : (d.n + 2047) / 2048);
  hipLaunchKernelGGL(k_mlr_predict<K>, dim3(bx, B), dim3(256), 0, st, d, coef, r);
}

#define SC_MLR_DISPATCH(fn, ...)                  \
  switch (a->k) {                                 \
    case 1: fn<1>(__VA_ARGS__); break;            \
    case 2: fn<2>(__VA_ARGS__); break;            \
    case 3: fn<3>(__VA_ARGS__); break;            \
    case 4: fn<4>(__VA_ARGS__); break;            \
    case 5: fn<5>(__VA_ARGS__); break;            \
    case 6: fn<6>(__VA_ARGS__); break;            \
    case 7: fn<7>(__VA_ARGS__); break;            \
    case 8: fn<8>(__VA_ARGS__); break;            \
    default: fn<9>(__VA_ARGS__); break;           \
  }

}  // namespace

extern "C" size_t sc_mlr_workspace_bytes(int B, size_t n, int k) {
  (void)k;
  const size_t G = mlr_groups(n);
  return al256((size_t)B * G * NM_MAX * sizeof(double)) + al256((size_t)B * G * 3 * sizeof(double)) +
         al256((size_t)2 * B * sizeof(double)) + al256(sc_trimmed_sum_workspace_bytes(B)) + (size_t)B * n * sizeof(float);
}

extern "C" int sc_mlr_moments(const sc_mlr_args* a, void* work, size_t work_bytes, sc_stream stream) {
  if (int rc = check_args(a, "sc_mlr_moments")) return rc;
  SC_REQUIRE(work && work_bytes >= sc_mlr_workspace_bytes(a->B, a->n, a->k), "sc_mlr_moments: workspace too small");
  const MlrD d = to_mlrd(*a);
  bool vec = ((uintptr_t)a->base % 16 == 0) && ((uintptr_t)a->target % 16 == 0) && a->tile_stride % 4 == 0 &&
             a->target_tile_stride % 4 == 0;
  for (int j = 0; j < a->k; ++j) vec = vec && a->band_off[j] % 4 == 0;
  MlrWork w = carve(work, a->B, a->n);
  SC_MLR_DISPATCH(launch_moments, d, a->B, vec ? 1 : 0, w.part, (hipStream_t)stream);
  SC_LAUNCH_OK("sc_mlr_moments");
  return SC_OK;
}

extern "C" int sc_mlr_solve(const sc_mlr_args* a, double* coef, void* work, size_t work_bytes, sc_stream stream) {
  if (int rc = check_args(a, "sc_mlr_solve")) return rc;
  SC_REQUIRE(coef && work && work_bytes >= sc_mlr_workspace_bytes(a->B, a->n, a->k), "sc_mlr_solve: bad argument");
  MlrWork w = carve(work, a->B, a->n);
  hipLaunchKernelGGL(k_mlr_solve, dim3(a->B), dim3(64), 0, (hipStream_t)stream, to_mlrd(*a), (const double*)w.part,
                     (int)mlr_groups(a->n), coef);
  SC_LAUNCH_OK("sc_mlr_solve");
  return SC_OK;
}

extern "C" int sc_mlr_fit(const sc_mlr_args* a, double* coef, void* work, size_t work_bytes, sc_stream stream) {
  if (int rc = sc_mlr_moments(a, work, work_bytes, stream)) return rc;
  return sc_mlr_solve(a, coef, work, work_bytes, stream);
}

extern "C" int sc_mlr_predict(const sc_mlr_args* a, const double* coef, float* r, sc_stream stream) {
  if (int rc = check_args(a, "sc_mlr_predict")) return rc;
  SC_REQUIRE(coef && r, "sc_mlr_predict: bad argument");
  const MlrD d = to_mlrd(*a);
  SC_MLR_DISPATCH(launch_predict, d, a->B, coef, r, (hipStream_t)stream);
  SC_LAUNCH_OK("sc_mlr_predict");
  return SC_OK;
}

extern "C" int sc_mlr_ratio(const sc_mlr_args* a, const double* coef, const float* r, int division, int autoclip, float* out, void* work,
                            size_t work_bytes, sc_stream stream) {
  if (int rc = check_args(a, "sc_mlr_ratio")) return rc;
  SC_REQUIRE(coef && out && work && work_bytes >= sc_mlr_workspace_bytes(a->B, a->n, a->k), "sc_mlr_ratio: bad argument");
  SC_REQUIRE(r || division != SC_MLR_C_MATCHED, "sc_mlr_ratio: c_matched_outliers needs the prediction r");
  SC_REQUIRE(division == SC_MLR_C_MATCHED || division == SC_MLR_SIMPLE_PLUS || division == SC_MLR_RESIDUAL,
             "sc_mlr_ratio: unknown division %d", division);
  hipStream_t st = (hipStream_t)stream;
  const MlrD d = to_mlrd(*a);
  MlrWork w = carve(work, a->B, a->n);
  const int B = a->B;
  const size_t n = a->n;
  if (division == SC_MLR_C_MATCHED) {
    const float* t = a->target;
    if (a->target_tile_stride != (long long)n && B > 1) {
      if (hipMemcpy2DAsync(w.tcopy, n * sizeof(float), a->target, (size_t)a->target_tile_stride * sizeof(float), n * sizeof(float),
                           (size_t)B, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        sc_set_error("sc_mlr_ratio: target copy failed"); return SC_ERR_LAUNCH;
      }
      t = w.tcopy;
    }
    if (int rc = sc_trimmed_sums(t, B, n, 5.0, w.sums, w.trim, w.trim_bytes, stream)) return rc;
    if (int rc = sc_trimmed_sums(r, B, n, 5.0, w.sums + B, w.trim, w.trim_bytes, stream)) return rc;
  } else if (division == SC_MLR_SIMPLE_PLUS) {
    SC_MLR_DISPATCH(launch_sp_stats, d, B, coef, w.sp, st);
    SC_LAUNCH_OK("sc_mlr_ratio(statistics)");
  }
  SC_MLR_DISPATCH(launch_ratio, d, B, coef, r, division, (const double*)w.sums, (const double*)w.sp, autoclip ? 1 : 0, out, st);
  SC_LAUNCH_OK("sc_mlr_ratio");
  return SC_OK;
}
