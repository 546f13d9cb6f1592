// Spectral-response-function band simulation (starcop/data/aviris.py:262-331 transform_to_srf, driven per band and per 50-column
// window by starcop/process_aviris.py:26-90 aviris_as_sensor): every output band j is a sparse weighted sum over AVIRIS bands,
//   out[j][l][s] = sum_{k in support(j)} w[j][k] * x[l][s][k]     (fill where any x[l][s][k] == fill, k in support(j))
// for all output bands in ONE launch, so the cube is read once instead of once per band.
//   band-contiguous (band stride 1: ENVI BIP, a (H, W, C) tensor): a work-group stages the band window [b0, b1] of the CSR for 64
//     consecutive samples of one line into LDS with 16-byte loads (window spans of neighbouring pixels share no granule reads
//     outside [b0, b1] beyond the 16-byte rounding), then each wave computes a quarter of the output bands with one lane per pixel;
//   strided (any other layout; sample stride 1 -- BSQ, BIL, a (C, H, W) tensor -- is the coalesced case): one lane per pixel, lanes
//     along samples, each support band's row read directly.
// Arithmetic: what numpy does with float64 weights times a float32 stack summed over axis 0 -- each product rounded to fp64 (the
// float32 value promoted exactly), added one at a time in ascending band order onto numpy's +0.0 seed (the additive identity its
// reduction starts from: a support of -0.0 values gives +0.0, as the reference does), rounded once to float32; never an FMA (see
// srf_pixel).  No atomics: repeated calls give identical bits.
#include <limits.h>

#include "sc_common.h"

namespace {

constexpr int SRF_NOUT_MAX = 64;
constexpr int SRF_TP = 64;                 // pixels per work-group of the band-contiguous path: one per lane
constexpr int SRF_WG = 256;                // four waves; wave v computes output bands v, v + 4, ...
constexpr int SRF_LDS_MAX = 160 * 1024;
constexpr int SRF_STAGE = 8;               // 16-byte loads in flight per thread while staging

struct SrfD {
  const float* x;
  long long ls, ss, bs;      // element strides of line, sample, band
  long long extent;          // 1 + offset of the last cube element: loads stay inside [0, extent)
  int L, S, n_out, b0, nb;   // nb = b1 - b0 + 1
  const int32_t* ptr;
  const int32_t* band;
  const double* w;
  float* out;
  long long ops, ols;        // output plane / line strides (elements); sample stride 1
  int has_fill;
  float fill;
};

// output band j of one pixel; get(b) = value of AVIRIS band b.  j is wave-uniform, so the CSR reads are scalar loads.
// HIP's __dmul_rn / __dadd_rn are plain operators that hipcc still contracts into v_fma_f64 (-ffp-contract=fast is its default), so
// the products and sums are written here under a scoped contract(off).
template <class Get>
__device__ __forceinline__ float srf_pixel(const SrfD& a, int j, Get get) {
#pragma clang fp contract(off)
  const int k0 = a.ptr[j], k1 = a.ptr[j + 1];
  bool bad = false;
  double acc = 0.0;
#pragma unroll 4
  for (int k = k0; k < k1; ++k) {
    const float v = get(a.band[k]);
    bad |= v == a.fill;
    const double p = a.w[k] * (double)v;
    acc = acc + p;
  }
  return (a.has_fill && bad) ? a.fill : __double2float_rn(acc);
}

// grid.x = L * tiles of 64 samples; LDS [64][sp] floats, sp odd (>= nb) so lanes reading one band hit distinct banks
template <bool VEC>
__global__ __launch_bounds__(SRF_WG) void k_srf_bip(SrfD a, int tiles, int sp) {
  extern __shared__ __attribute__((aligned(16))) float win[];
  const int l = blockIdx.x / tiles;
  const int s0 = (blockIdx.x - l * tiles) * SRF_TP;
  const int np = min(SRF_TP, a.S - s0);
  const long long base = (long long)l * a.ls + (long long)s0 * a.ss + a.b0;      // window start of pixel s0
  if (VEC) {
    // pixel i's window [a0, a0 + nb) lies in at most ng 16-byte granules; consecutive threads take consecutive granules.  Each
    // thread issues SRF_STAGE loads before it writes any of them to LDS: one load in flight per thread left the 4 waves of a CU
    // waiting on HBM latency for most of the kernel.
    const int ng = (a.nb + 6) >> 2;
    const int total = np * ng;
    for (int q0 = threadIdx.x; q0 < total; q0 += SRF_WG * SRF_STAGE) {
      float4 v[SRF_STAGE];
      long long g[SRF_STAGE], a0[SRF_STAGE];
      int row[SRF_STAGE];
#pragma unroll
      for (int u = 0; u < SRF_STAGE; ++u) {
        const int q = q0 + u * SRF_WG;
        const int i = q < total ? q / ng : 0;
        row[u] = q < total ? i : -1;
        a0[u] = base + (long long)i * a.ss;
        g[u] = ((a0[u] >> 2) + (q - i * ng)) << 2;
        if (q < total && g[u] < a0[u] + a.nb && g[u] + 4 <= a.extent) v[u] = *reinterpret_cast<const float4*>(a.x + g[u]);
      }
#pragma unroll
      for (int u = 0; u < SRF_STAGE; ++u) {
        if (row[u] < 0 || g[u] >= a0[u] + a.nb) continue;
        float* dst = win + row[u] * sp;
        const bool whole = g[u] + 4 <= a.extent;
        const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const long long kk = g[u] + t - a0[u];
          if (kk >= 0 && kk < a.nb) dst[kk] = whole ? e[t] : a.x[g[u] + t];
        }
      }
    }
  } else {
    for (int q = threadIdx.x; q < np * a.nb; q += SRF_WG) {
      const int i = q / a.nb, kk = q - i * a.nb;
      win[i * sp + kk] = a.x[base + (long long)i * a.ss + kk];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (lane >= np) return;
  const float* px = win + lane * sp - a.b0;
  float* o = a.out + (long long)l * a.ols + s0 + lane;
  for (int j = wave; j < a.n_out; j += SRF_WG / 64) o[(long long)j * a.ops] = srf_pixel(a, j, [&](int b) { return px[b]; });
}

// grid.x = L * tiles of 256 samples
__global__ __launch_bounds__(SRF_WG) void k_srf_strided(SrfD a, int tiles) {
  const int l = blockIdx.x / tiles;
  const int s = (blockIdx.x - l * tiles) * SRF_WG + threadIdx.x;
  if (s >= a.S) return;
  const float* px = a.x + (long long)l * a.ls + (long long)s * a.ss;
  float* o = a.out + (long long)l * a.ols + s;
  for (int j = 0; j < a.n_out; ++j) o[(long long)j * a.ops] = srf_pixel(a, j, [&](int b) { return px[(long long)b * a.bs]; });
}

template <bool VEC>
int launch_bip(const SrfD& d, int tiles, int sp, size_t lds, hipStream_t st) {
  SC_REQUIRE(sc_lds_limit(&k_srf_bip<VEC>, lds, "sc_srf_bands") == SC_OK, "sc_srf_bands: cannot raise the LDS limit of the band-contiguous kernel");
  hipLaunchKernelGGL(k_srf_bip<VEC>, dim3((unsigned)d.L * (unsigned)tiles), dim3(SRF_WG), lds, st, d, tiles, sp);
  return SC_OK;
}

}  // namespace

extern "C" int sc_srf_bands(const sc_srf_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_srf_bands: null arguments");
  SC_REQUIRE(a->x && a->out && a->ptr && a->band && a->w && a->ptr_host && a->band_host, "sc_srf_bands: null pointer");
  SC_REQUIRE(a->L >= 1 && a->S >= 1 && a->B >= 1, "sc_srf_bands: bad cube dims L=%d S=%d B=%d", a->L, a->S, a->B);
  SC_REQUIRE(a->line_stride >= 0 && a->sample_stride >= 0 && a->band_stride >= 0 && a->out_plane_stride >= 0 &&
                 a->out_line_stride >= 0, "sc_srf_bands: negative stride");
  SC_REQUIRE(a->n_out >= 1 && a->n_out <= SRF_NOUT_MAX, "sc_srf_bands: n_out=%d outside [1, %d]", a->n_out, SRF_NOUT_MAX);
  SC_REQUIRE(a->ptr_host[0] == 0, "sc_srf_bands: ptr[0]=%d, expected 0", a->ptr_host[0]);
  int b0 = a->B, b1 = -1;
  for (int j = 0; j < a->n_out; ++j) {
    const int k0 = a->ptr_host[j], k1 = a->ptr_host[j + 1];
    SC_REQUIRE(k1 > k0, "sc_srf_bands: output band %d has no weights", j);
    for (int k = k0; k < k1; ++k) {
      const int b = a->band_host[k];
      SC_REQUIRE(b >= 0 && b < a->B, "sc_srf_bands: band index %d outside [0, %d)", b, a->B);
      SC_REQUIRE(k == k0 || b > a->band_host[k - 1], "sc_srf_bands: band indices of output band %d are not ascending", j);
    }
    b0 = min(b0, a->band_host[k0]);
    b1 = max(b1, a->band_host[k1 - 1]);
  }
  SrfD d;
  d.x = a->x; d.ls = a->line_stride; d.ss = a->sample_stride; d.bs = a->band_stride;
  d.extent = 1 + (long long)(a->L - 1) * d.ls + (long long)(a->S - 1) * d.ss + (long long)(a->B - 1) * d.bs;
  d.L = a->L; d.S = a->S; d.n_out = a->n_out; d.b0 = b0; d.nb = b1 - b0 + 1;
  d.ptr = a->ptr; d.band = a->band; d.w = a->w;
  d.out = a->out; d.ops = a->out_plane_stride; d.ols = a->out_line_stride;
  d.has_fill = a->has_fill ? 1 : 0; d.fill = a->fill;
  hipStream_t st = (hipStream_t)stream;
  const int sp = d.nb | 1;
  const size_t lds = (size_t)SRF_TP * sp * sizeof(float);
  if ((a->band_stride == 1 || a->B == 1) && lds <= (size_t)SRF_LDS_MAX) {
    const int tiles = (a->S + SRF_TP - 1) / SRF_TP;
    SC_REQUIRE((long long)tiles * a->L <= INT_MAX, "sc_srf_bands: cube too large for one launch");
    const int rc = ((uintptr_t)a->x % 16 == 0) ? launch_bip<true>(d, tiles, sp, lds, st) : launch_bip<false>(d, tiles, sp, lds, st);
    if (rc) return rc;
  } else {
    const int tiles = (a->S + SRF_WG - 1) / SRF_WG;
    SC_REQUIRE((long long)tiles * a->L <= INT_MAX, "sc_srf_bands: cube too large for one launch");
    hipLaunchKernelGGL(k_srf_strided, dim3((unsigned)a->L * (unsigned)tiles), dim3(SRF_WG), 0, st, d, tiles);
  }
  SC_LAUNCH_OK("sc_srf_bands");
  return SC_OK;
}
