// Label sums of the training windows of every resident tile (starcop/data/datamodule.py:17-64, tiled_dataframe: the
// frac_positives column is torch.sum(label window) / window size, one DataLoader item per window in the reference):
//   out[m][k] = sum over the window k = (row_off, col_off, height, width) of tile m of labels[m][r][c], accumulated in fp64.
// The window table is shared by all tiles; windows may overlap, repeat, be one pixel or the whole tile.
//   Mapping: one work-group of 256 threads owns one (tile, window) pair, so a pixel is read once per window that covers it (up to
//   four times on the 128 / 64 grid).  The re-reads stay on chip: a 512 x 512 tile is 1 MiB and the launch is ordered so that the
//   K windows of a tile are consecutive work-groups of ONE XCD (block b runs on XCD b mod 8; it takes the pair
//   (b mod 8) * ceil(M*K / 8) + b / 8), i.e. they meet in that XCD's 4 MiB L2.  This is a placement hint only: nothing depends on it.
//   Inside the work-group the threads form an LX x LY grid (LX = the power of two >= the 16-byte vectors of a row segment, at
//   most 256): thread (tx, ty) walks rows ty, ty + LY, .. and vectors tx, tx + LX, ..  A row segment is cut at the 16-byte
//   boundaries of the ARRAY (rows of a tile whose width is no multiple of 4 change their alignment from row to row): a vector
//   that lies inside the window whole is one 16-byte load, the ragged ends are read element by element, nothing outside the
//   window is dereferenced.  When `labels` itself is not 16-byte aligned every vector is one element.
//   Order of the additions: each thread adds its elements in walk order into four fp64 partials (row ty + 4q*LY.. into partial q
//   modulo 4), folds them ((p0 + p1) + (p2 + p3)), the wave adds across lanes with the xor butterfly (32, 16, .., 1), wave sums
//   go through LDS and thread 0 adds them in wave order.  No atomics: repeated calls give identical bits, and any window whose
//   partial sums are integers below 2^53 ({0, 1} labels at every possible size) is summed exactly.
//   The kernel re-checks its window against the tile before it reads (a device table that differs from the checked host table
//   yields NaN for that window, never an out-of-bounds read).
#include <limits.h>

#include "sc_common.h"

namespace {

constexpr int TSUM_WG = 256;
constexpr int TSUM_XCDS = 8;

struct TsumD {
  const float* x;
  const int32_t* win;      // [K][4] (row_off, col_off, height, width)
  double* out;             // [M][K]
  int H, W, K;
  unsigned total, per_xcd; // M * K pairs, ceil(total / 8)
  int vec;                 // elements per vector: 4 (x is 16-byte aligned) or 1
};

template <int V>
__device__ __forceinline__ double tsum_vec(const float* __restrict__ x, long long e, long long s, long long end) {
  // elements [e, e + V) of the array, of which [s, end) belong to the window's row segment
  if constexpr (V == 4) {
    if (e >= s && e + 4 <= end) {
      const float4 v = *reinterpret_cast<const float4*>(x + e);
      return (((double)v.x + (double)v.y) + (double)v.z) + (double)v.w;
    }
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e + u >= s && e + u < end) a += (double)x[e + u];
    return a;
  } else {
    return (double)x[e];
  }
}

template <int V>
__global__ __launch_bounds__(TSUM_WG) void k_tile_window_sums(TsumD a) {
  __shared__ double part[TSUM_WG / 64];
  const unsigned pair = (blockIdx.x % TSUM_XCDS) * a.per_xcd + blockIdx.x / TSUM_XCDS;
  if (pair >= a.total) return;                                  // uniform: the whole work-group leaves
  const unsigned m = pair / (unsigned)a.K, k = pair - m * (unsigned)a.K;
  const int r0 = a.win[4 * (size_t)k], c0 = a.win[4 * (size_t)k + 1], h = a.win[4 * (size_t)k + 2], w = a.win[4 * (size_t)k + 3];
  if (r0 < 0 || c0 < 0 || h < 1 || w < 1 || (long long)r0 + h > a.H || (long long)c0 + w > a.W) {
    if (threadIdx.x == 0) a.out[pair] = __builtin_nan("");
    return;
  }
  const long long W = a.W;
  const long long first = ((long long)m * a.H + r0) * W + c0;   // array index of the window's first element
  // vectors per row segment: exact where every row shares the alignment of the first, else the bound that covers all of them
  int nv;
  if (V == 1) nv = w;
  else if ((W & 3) == 0) nv = (int)(((first + w + 3) >> 2) - (first >> 2));
  else nv = ((w + 3) >> 2) + 1;
  int lx = 1;
  while (lx < nv && lx < TSUM_WG) lx <<= 1;
  const int ly = TSUM_WG / lx;
  const int tx = (int)threadIdx.x & (lx - 1), ty = (int)threadIdx.x / lx;
  double p[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i0 = ty; i0 < h; i0 += 4 * ly) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * ly;
      if (i < h) {
        const long long s = first + (long long)i * W, end = s + w;
        const long long base = V == 4 ? (s & ~3ll) : s;
        for (int j = tx; j < nv; j += lx) {
          const long long e = base + (long long)j * V;
          if (e < end) p[q] += tsum_vec<V>(a.x, e, s, end);
        }
      }
    }
  }
  double v = wave_sum_d((p[0] + p[1]) + (p[2] + p[3]));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = part[0];
#pragma unroll
    for (int q = 1; q < TSUM_WG / 64; ++q) t += part[q];
    a.out[pair] = t;
  }
}

}  // namespace

extern "C" int sc_tile_window_sums(const float* labels, int M, int H, int W, const int32_t* windows, const int32_t* windows_host, int K,
                                   double* out, sc_stream stream) {
  SC_REQUIRE(labels && windows && windows_host && out, "sc_tile_window_sums: null pointer");
  SC_REQUIRE(M >= 1, "sc_tile_window_sums: no tiles (M=%d)", M);
  SC_REQUIRE(K >= 1, "sc_tile_window_sums: empty window table (K=%d)", K);
  SC_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "sc_tile_window_sums: bad tile dims H=%d W=%d", H, W);
  SC_REQUIRE((uintptr_t)labels % 4 == 0 && (uintptr_t)windows % 4 == 0 && (uintptr_t)out % 8 == 0, "sc_tile_window_sums: misaligned pointer");
  const long long total = (long long)M * K;
  const long long per_xcd = (total + TSUM_XCDS - 1) / TSUM_XCDS;
  SC_REQUIRE(per_xcd * TSUM_XCDS <= INT_MAX, "sc_tile_window_sums: %lld (tile, window) pairs are too many for one launch", total);
  for (int i = 0; i < K; ++i) {
    const int32_t* q = windows_host + (size_t)i * 4;
    SC_REQUIRE(q[2] >= 1 && q[3] >= 1, "sc_tile_window_sums: window %d has height %d, width %d", i, q[2], q[3]);
    SC_REQUIRE(q[0] >= 0 && q[1] >= 0 && (long long)q[0] + q[2] <= H && (long long)q[1] + q[3] <= W,
               "sc_tile_window_sums: window %d (row %d, col %d, %d x %d) leaves the %d x %d tile", i, q[0], q[1], q[2], q[3], H, W);
  }
  TsumD d;
  d.x = labels; d.win = windows; d.out = out; d.H = H; d.W = W; d.K = K;
  d.total = (unsigned)total; d.per_xcd = (unsigned)per_xcd;
  d.vec = (uintptr_t)labels % 16 == 0 ? 4 : 1;
  const dim3 grid((unsigned)(per_xcd * TSUM_XCDS));
  if (d.vec == 4) hipLaunchKernelGGL((k_tile_window_sums<4>), grid, dim3(TSUM_WG), 0, (hipStream_t)stream, d);
  else hipLaunchKernelGGL((k_tile_window_sums<1>), grid, dim3(TSUM_WG), 0, (hipStream_t)stream, d);
  SC_LAUNCH_OK("sc_tile_window_sums");
  return SC_OK;
}
