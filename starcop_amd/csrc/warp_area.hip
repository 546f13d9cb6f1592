// Footprint resampling for the warp (sc_warp_area, include/starcop_hip.h): average, max, min and mode of the source pixels under a
// destination pixel's footprint, for destinations coarser than their source.  Per destination pixel, all in fp64:
//   1. the four corners through the arithmetic of warp.hip's centre (destination affine, CRS route, inverse source affine), unclipped,
//   2. their axis-aligned bounding box [u0, u1] x [v0, v1] in source pixel coordinates, its area A, the box clipped to the raster,
//   3. per source column / row the overlap wx / wy with the clipped box; a pixel takes part when both exceed 2^-20 (the sliver rule),
//   4. per plane the reduction over the samples that count (not the no-data pattern, not NaN), the coverage sum w / A and the
//      footprint rule coverage >= min_coverage.
//   Corner lattice: a work-group projects the (TY + 1) x (TX + 1) corners of its tile ONCE into LDS (two fp64 series each); every
//   pixel reads its four from there: 289 / 256 = 1.13 projections per pixel on the 16 x 16 tile instead of 4.  Box, clip and the
//   column range are computed once per pixel and kept in registers over the plane loop.
//   Two mappings, chosen on the host from the box width of the destination's corner pixels (area_variant below):
//   k_area_thread: one thread per destination pixel (4 consecutive pixels of a row with 16-byte stores) loops over its box.  For boxes
//     of a few source pixels: neighbouring threads' boxes touch, the cache serves the reads.  On a 12 x 12 box every lane would stride
//     48 bytes from its neighbour, which is what the other mapping is for.
//   k_area_lanes: 16 lanes own one destination pixel and run along source columns (lane l: columns j0 + l, j0 + l + 16, ...), rows
//     in a loop; the 4 groups of a wave own 4 ADJACENT pixels of a destination row, whose boxes are adjacent in the source, so a wave
//     reads one contiguous segment per source row.  Every lane accumulates its samples column by column, rows ascending, then a fixed xor-butterfly
//     (8, 4, 2, 1) inside the group combines them: every lane ends with the same bits (fp64 addition commutes), lane 0 of the wave
//     collects the 4 results and stores them as one 16-byte word.  The `mode` tally is a 256-bin histogram per group in LDS, integer
//     atomics only; the lanes of a group meet at wave-level fences, never at a work-group barrier, because loop bounds differ per group.
//   Reduction order is fixed in both: two calls give the same bytes.  max / min / mode do not depend on the order at all (integer
//   keys), so the mappings agree bit for bit; `average` differs by the fp64 summation order.  No loop waits on another work-group.
#include <limits.h>
#include <math.h>

#include <cmath>

#include "sc_common.h"
#include "sc_warp.h"

namespace {

constexpr int AREA_PMAX = SC_WARP_MAX_PLANES;
constexpr int AREA_WG = 256;
constexpr int AREA_T = 16;                       // tile edge in pixels (both mappings; the 16-byte-store thread tile is 16 x 64)
constexpr double AREA_SLIVER = 1.0 / 1048576.0;  // 2^-20: an overlap at or below it does not take part
#ifndef AREA_ROWS
#define AREA_ROWS 8                               // source rows a lane of k_area_lanes loads before it uses the first
#endif
#ifndef AREA_LANES_WG
#define AREA_LANES_WG 256                         // threads of a k_area_lanes work-group: 4 waves of 4 tile rows each
#endif
// Measured (tools/bench_warp_area.py -> profiles/warp_area.txt, 9000 x 4000 x 5 planes onto 60 m, average, aligned | geographic case):
// 1 row in flight 1211 | 1353 us, 4 rows 600 | 663 us, 8 rows 478 | 544 us, 12 rows 548 | 628 us; 512 threads with 8 rows 486 | 566 us.
// Box width in source columns from which the lane-group mapping is chosen.  Measured at ONE width only (profiles/warp_area.txt, boxes
// of 12 to 14 columns): there the lane groups take 0.12 x the time of the thread mapping for `mode` of a uint8 mask, 0.29 x for
// `average` when the thread mapping runs its 16-byte-store form (4 pixels per thread), and 1.17 x -- they lose -- against its
// one-pixel form (a destination width that is no multiple of 4).  Where between 1 and 12 columns the two cross has NOT been measured:
// 4.0 only separates boxes of a pixel or two from boxes of a dozen columns.
constexpr double AREA_LANES_FROM_WIDTH = 4.0;

enum { K_AVG = 0, K_EXT = 1, K_MODE = 2 };

struct AreaD {
  double gt[6], inv[6];
  Krueger k;
  double dst_lon0, dst_fn, src_lon0, src_fn;
  double min_cov;
  int route;                                     // bit 0: destination is UTM (inverse first), bit 1: source is UTM (forward after)
  int H, W, sh, sw, P, tiles_x;
  uint32_t flip;                                 // K_EXT: 0 = max, ~0 = min (the key is complemented)
  void* out;
  float* cov;
  double* boxes;
  const void* src[AREA_PMAX];
  long long rs[AREA_PMAX], cs[AREA_PMAX];
  unsigned long long nod[AREA_PMAX];
};

// source pixel coordinates of the destination lattice point (px, py), unclipped; false when the projection has no finite result
__host__ __device__ __forceinline__ bool corner_uv(const AreaD& a, double px, double py, double& u, double& v) {
  return grid_uv(a, px, py, u, v) && fabs(u) < INFINITY && fabs(v) < INFINITY;      // false for NaN too
}

// the corners (y0 .. y0 + LH - 1) x (x0 .. x0 + LW - 1) of a tile into LDS; NaN for a corner without coordinates or beyond the grid
template <int LH, int LW>
__device__ __forceinline__ void project_lattice(const AreaD& a, int y0, long long x0, double (*lu)[LW], double (*lv)[LW]) {
  for (int i = threadIdx.x; i < LH * LW; i += blockDim.x) {
    const int r = i / LW, c = i - r * LW;
    double u = __builtin_nan(""), v = u;
    if (y0 + r <= a.H && x0 + c <= a.W && !corner_uv(a, (double)(x0 + c), (double)(y0 + r), u, v)) u = v = __builtin_nan("");
    lu[r][c] = u;
    lv[r][c] = v;
  }
  __syncthreads();
}

// what the planes share about one destination pixel
struct Foot {
  double u0, u1, v0, v1;                         // the unclipped box; NaN when a corner has no coordinates
  double cu0, cu1, cv0, cv1, A;                  // the clipped box and the unclipped area
  int j0, j1, i0, i1;                            // source columns / rows [floor(c?0), ceil(c?1)); empty when the pixel is no-data
};

template <int LW>
__device__ __forceinline__ Foot footprint(const AreaD& a, const double (*lu)[LW], const double (*lv)[LW], int r, int c) {
  const double ua = lu[r][c], ub = lu[r][c + 1], uc = lu[r + 1][c], ud = lu[r + 1][c + 1];
  const double va = lv[r][c], vb = lv[r][c + 1], vc = lv[r + 1][c], vd = lv[r + 1][c + 1];
  Foot f;
  f.j0 = f.j1 = f.i0 = f.i1 = 0;
  f.cu0 = f.cu1 = f.cv0 = f.cv1 = 0.0;
  f.A = 1.0;
  if (!(ua == ua && ub == ub && uc == uc && ud == ud)) {      // u and v of a corner are NaN together
    f.u0 = f.u1 = f.v0 = f.v1 = __builtin_nan("");
    return f;
  }
  f.u0 = fmin(fmin(ua, ub), fmin(uc, ud)); f.u1 = fmax(fmax(ua, ub), fmax(uc, ud));
  f.v0 = fmin(fmin(va, vb), fmin(vc, vd)); f.v1 = fmax(fmax(va, vb), fmax(vc, vd));
  f.A = (f.u1 - f.u0) * (f.v1 - f.v0);
  f.cu0 = fmax(f.u0, 0.0); f.cu1 = fmin(f.u1, (double)a.sw);
  f.cv0 = fmax(f.v0, 0.0); f.cv1 = fmin(f.v1, (double)a.sh);
  if (f.cu0 < f.cu1 && f.cv0 < f.cv1) {
    f.j0 = (int)floor(f.cu0); f.j1 = (int)ceil(f.cu1);
    f.i0 = (int)floor(f.cv0); f.i1 = (int)ceil(f.cv1);
  }
  return f;
}

__device__ __forceinline__ void store_box(const AreaD& a, const Foot& f, size_t pix) {
  const size_t plane = (size_t)a.H * a.W;
  a.boxes[pix] = f.u0;
  a.boxes[plane + pix] = f.u1;
  a.boxes[2 * plane + pix] = f.v0;
  a.boxes[3 * plane + pix] = f.v1;
}

// a sample counts; its integer key in the order of the values (float32: sign-magnitude -> unsigned, -0 < +0)
template <class T>
__device__ __forceinline__ bool sample_counts(T b, T nod) {
  if constexpr (sizeof(T) == 4) return counts(b, nod);
  else return b != nod;
}
template <class T>
__device__ __forceinline__ uint32_t key_of(T b) {
  if constexpr (sizeof(T) == 4) return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  else return b;
}
template <class T>
__device__ __forceinline__ T of_key(uint32_t k) {
  if constexpr (sizeof(T) == 4) return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  else return (T)k;
}

// what one lane (or one thread) has gathered of one plane
struct Part {
  double acc, wsum;                              // sum w x (K_AVG), sum w over counting samples
  unsigned long long best;                       // K_EXT: 2^32 + the largest key; K_MODE: count << 8 | 255 - value; 0 = nothing
};

// the value and the coverage of a pixel from the combined parts: no-data unless a sample counts and the coverage suffices
template <class T, int KIND>
__device__ __forceinline__ T finish(const AreaD& a, const Part& s, double A, T nod, float& cov) {
  const double c = s.wsum / A;
  cov = 0.f;
  if (!(s.wsum > 0.0 && c >= a.min_cov)) return nod;
  cov = (float)c;
  if constexpr (KIND == K_AVG) return __float_as_uint((float)(s.acc / s.wsum));
  else if constexpr (KIND == K_EXT) return of_key<T>((uint32_t)s.best ^ a.flip);
  else return (T)(255u - (uint32_t)(s.best & 0xFFu));
}

// ---------------------------------------------------------------------------------------------------------- one thread per pixel
template <class T, int KIND>
__device__ __forceinline__ Part reduce_thread(const T* s, long long rs, long long cs, T nod, uint32_t flip, const Foot& f) {
  Part r = {0.0, 0.0, 0ull};
  unsigned long long seen0 = 0, seen1 = 0, seen2 = 0, seen3 = 0;      // K_MODE: the values that have been tallied
  for (int i = f.i0; i < f.i1; ++i) {
    const double wy = fmin((double)i + 1.0, f.cv1) - fmax((double)i, f.cv0);
    if (!(wy > AREA_SLIVER)) continue;
    for (int j = f.j0; j < f.j1; ++j) {
      const double wx = fmin((double)j + 1.0, f.cu1) - fmax((double)j, f.cu0);
      if (!(wx > AREA_SLIVER)) continue;
      const T b = s[i * rs + j * cs];
      if (!sample_counts<T>(b, nod)) continue;
      const double w = wx * wy;
      r.wsum += w;
      if constexpr (KIND == K_AVG) r.acc += w * (double)__uint_as_float(b);
      if constexpr (KIND == K_EXT) {
        const unsigned long long k = 0x100000000ull | (key_of<T>(b) ^ flip);
        r.best = k > r.best ? k : r.best;
      }
      if constexpr (KIND == K_MODE) {
        // without a histogram of its own a thread counts the box again for every value it meets for the first time: samples x
        // distinct values, for the few samples this mapping is chosen for
        const unsigned q = b >> 6;
        const unsigned long long bit = 1ull << (b & 63u);
        if ((q == 0 ? seen0 : q == 1 ? seen1 : q == 2 ? seen2 : seen3) & bit) continue;
        seen0 |= q == 0 ? bit : 0ull; seen1 |= q == 1 ? bit : 0ull; seen2 |= q == 2 ? bit : 0ull; seen3 |= q == 3 ? bit : 0ull;
        unsigned long long n = 0;
        for (int ii = f.i0; ii < f.i1; ++ii) {
          if (!(fmin((double)ii + 1.0, f.cv1) - fmax((double)ii, f.cv0) > AREA_SLIVER)) continue;
          for (int jj = f.j0; jj < f.j1; ++jj) {
            if (!(fmin((double)jj + 1.0, f.cu1) - fmax((double)jj, f.cu0) > AREA_SLIVER)) continue;
            n += s[ii * rs + jj * cs] == b ? 1u : 0u;
          }
        }
        const unsigned long long k = n << 8 | (255u - b);
        r.best = k > r.best ? k : r.best;
      }
    }
  }
  return r;
}

// grid.x = tiles_y * tiles_x tiles of 16 rows x TX * V pixels; a thread owns V consecutive pixels of a row
template <class T, int V, int KIND>
__global__ __launch_bounds__(AREA_WG) void k_area_thread(AreaD a) {
  constexpr int TX = V == 1 ? AREA_T : 16, TY = AREA_WG / TX, LW = TX * V + 1;
  __shared__ double lu[TY + 1][LW], lv[TY + 1][LW];
  const int by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  project_lattice<TY + 1, LW>(a, by * TY, (long long)bx * TX * V, lu, lv);
  const long long x0 = ((long long)bx * TX + tx) * V;
  const int y = by * TY + ty;
  if (y >= a.H || x0 >= a.W) return;              // W % V == 0 on the vector path
  const size_t pix = (size_t)y * a.W + (size_t)x0, plane = (size_t)a.H * a.W;
  Foot f[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    f[e] = footprint<LW>(a, lu, lv, ty, tx * V + e);
    if (a.boxes) store_box(a, f[e], pix + e);
  }
  T* o = static_cast<T*>(a.out) + pix;
  for (int p = 0; p < a.P; ++p) {
    const T* s = static_cast<const T*>(a.src[p]);
    const long long rs = a.rs[p], cs = a.cs[p];
    const T nod = (T)a.nod[p];
    Pack<T, V> r;
    Pack<float, V> c;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = finish<T, KIND>(a, reduce_thread<T, KIND>(s, rs, cs, nod, a.flip, f[e]), f[e].A, nod, c.v[e]);
    *reinterpret_cast<Pack<T, V>*>(o + (size_t)p * plane) = r;
    if (a.cov) *reinterpret_cast<Pack<float, V>*>(a.cov + (size_t)p * plane + pix) = c;
  }
}

// ---------------------------------------------------------------------------------------------------------- 16 lanes per pixel
__device__ __forceinline__ double xor_sum16(double v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, 16);
  return v;
}
__device__ __forceinline__ unsigned long long xor_max16(unsigned long long v) {
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 16);
    v = o > v ? o : v;
  }
  return v;
}

// the lanes of a wave have issued their LDS operations in program order; this keeps the compiler from moving one across
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// grid.x = tiles_y * tiles_x tiles of 16 x 16 pixels; a wave owns ROWS consecutive rows of the tile, in ROWS * 4 steps of 4 adjacent
// pixels.  VEC: one 16-byte (uint8: 4-byte) store per step and plane by lane 0; else the first lane of every group stores its pixel
template <class T, int KIND, bool VEC>
__global__ __launch_bounds__(AREA_LANES_WG) void k_area_lanes(AreaD a) {
  constexpr int LW = AREA_T + 1, ROWS = AREA_T / (AREA_LANES_WG / 64);
  static_assert(ROWS * (AREA_LANES_WG / 64) == AREA_T, "the waves of a work-group share the rows of a tile evenly");
  __shared__ double lu[LW][LW], lv[LW][LW];
  __shared__ unsigned hist[KIND == K_MODE ? AREA_LANES_WG / 16 : 1][KIND == K_MODE ? 256 : 1];
  const int by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64, g = lane / 16, l = lane % 16;
  if constexpr (KIND == K_MODE) {
    for (int i = threadIdx.x; i < (AREA_LANES_WG / 16) * 256; i += AREA_LANES_WG) (&hist[0][0])[i] = 0u;      // before the barrier of project_lattice
  }
  project_lattice<LW, LW>(a, by * AREA_T, (long long)bx * AREA_T, lu, lv);
  unsigned* h = hist[KIND == K_MODE ? threadIdx.x / 16 : 0];
  const size_t plane = (size_t)a.H * a.W;
  for (int q = 0; q < ROWS * 4; ++q) {
    const int ty = wave * ROWS + q / 4, txq = (q % 4) * 4;
    const int y = by * AREA_T + ty;
    const long long xq = (long long)bx * AREA_T + txq, x = xq + g;
    if (y >= a.H || xq >= a.W) continue;          // uniform over the wave
    const bool mine = x < a.W;                    // false only on the one-pixel path, for a group beyond the row's end
    Foot f = footprint<LW>(a, lu, lv, ty, txq + g);
    if (!mine) f.i1 = f.i0;
    const size_t pix = (size_t)y * a.W + (size_t)x;
    if (a.boxes && mine && l == 0) store_box(a, f, pix);
    for (int p = 0; p < a.P; ++p) {
      const T* s = static_cast<const T*>(a.src[p]);
      const long long rs = a.rs[p], cs = a.cs[p];
      const T nod = (T)a.nod[p];
      Part r = {0.0, 0.0, 0ull};
      for (int j = f.j0 + l; j < f.j1; j += 16) {
        const double wx = fmin((double)j + 1.0, f.cu1) - fmax((double)j, f.cu0);
        if (!(wx > AREA_SLIVER)) continue;
        const T* col = s + j * cs;
        // AREA_ROWS rows at a time: their loads are issued before the first is used, so a wave has that many row segments in flight
        // (a row past the box repeats the last one, which the cache holds, and is left out below)
        for (int i = f.i0; i < f.i1; i += AREA_ROWS) {
          T b[AREA_ROWS];
#pragma unroll
          for (int k = 0; k < AREA_ROWS; ++k) b[k] = col[(long long)min(i + k, f.i1 - 1) * rs];
#pragma unroll
          for (int k = 0; k < AREA_ROWS; ++k) {
            const int ii = i + k;
            const double wy = fmin((double)ii + 1.0, f.cv1) - fmax((double)ii, f.cv0);
            if (ii < f.i1 && wy > AREA_SLIVER && sample_counts<T>(b[k], nod)) {
              const double w = wx * wy;
              r.wsum += w;
              if constexpr (KIND == K_AVG) r.acc += w * (double)__uint_as_float(b[k]);
              if constexpr (KIND == K_EXT) {
                const unsigned long long key = 0x100000000ull | (key_of<T>(b[k]) ^ a.flip);
                r.best = key > r.best ? key : r.best;
              }
              if constexpr (KIND == K_MODE) atomicAdd(&h[b[k]], 1u);
            }
          }
        }
      }
      if constexpr (KIND == K_MODE) {
        wave_lds_fence();
        for (int k = 0; k < 16; ++k) {            // lane l reads (and clears for the next plane) bins l, 16 + l, ...: no bank twice
          const unsigned v = k * 16 + l, n = h[v];
          h[v] = 0u;
          const unsigned long long key = n ? (unsigned long long)n << 8 | (255u - v) : 0ull;
          r.best = key > r.best ? key : r.best;
        }
        wave_lds_fence();
      }
      r.wsum = xor_sum16(r.wsum);
      if constexpr (KIND == K_AVG) r.acc = xor_sum16(r.acc);
      else r.best = xor_max16(r.best);
      float c;
      const T val = finish<T, KIND>(a, r, f.A, nod, c);
      T* o = static_cast<T*>(a.out) + (size_t)p * plane + pix;
      float* oc = a.cov ? a.cov + (size_t)p * plane + pix : nullptr;
      if constexpr (VEC) {
        Pack<T, 4> rv;
        Pack<float, 4> cv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          rv.v[e] = (T)__shfl((unsigned)val, 16 * e);
          cv.v[e] = __shfl(c, 16 * e);
        }
        if (lane == 0) {
          *reinterpret_cast<Pack<T, 4>*>(o) = rv;
          if (oc) *reinterpret_cast<Pack<float, 4>*>(oc) = cv;
        }
      } else if (mine && l == 0) {
        *o = val;
        if (oc) *oc = c;
      }
    }
  }
}

template <class T, int KIND>
void launch(const AreaD& d0, int variant, bool vec, hipStream_t st) {
  AreaD d = d0;
  const int tw = (variant == SC_WARP_AREA_THREAD && vec) ? 64 : AREA_T;
  d.tiles_x = (d.W + tw - 1) / tw;
  const unsigned tiles = (unsigned)((long long)d.tiles_x * ((d.H + AREA_T - 1) / AREA_T));       // < 2^31 pixels: fits
  if (variant == SC_WARP_AREA_THREAD) {
    if (vec) hipLaunchKernelGGL((k_area_thread<T, 4, KIND>), dim3(tiles), dim3(AREA_WG), 0, st, d);
    else hipLaunchKernelGGL((k_area_thread<T, 1, KIND>), dim3(tiles), dim3(AREA_WG), 0, st, d);
  } else {
    if (vec) hipLaunchKernelGGL((k_area_lanes<T, KIND, true>), dim3(tiles), dim3(AREA_LANES_WG), 0, st, d);
    else hipLaunchKernelGGL((k_area_lanes<T, KIND, false>), dim3(tiles), dim3(AREA_LANES_WG), 0, st, d);
  }
}

// the mapping for a grid pair: the widest box, in source columns, of the destination's four corner pixels (host, the device's series)
int area_variant(const AreaD& d) {
  double width = 0.0;
  for (int k = 0; k < 4; ++k) {
    const double r = (k & 2) ? d.H - 1 : 0, c = (k & 1) ? d.W - 1 : 0;
    double lo = INFINITY, hi = -INFINITY;
    bool ok = true;
    for (int e = 0; e < 4; ++e) {
      double u, v;
      ok = corner_uv(d, c + (e & 1), r + (e >> 1), u, v) && ok;
      lo = fmin(lo, u); hi = fmax(hi, u);
    }
    if (ok) width = fmax(width, hi - lo);
  }
  return width >= AREA_LANES_FROM_WIDTH ? SC_WARP_AREA_LANES : SC_WARP_AREA_THREAD;
}

// checks everything but the device pointers' contents and fills the kernel's descriptor.  `launch`: the call will write something (the
// query of the mapping needs no output)
int prepare(const sc_warp_area_args* a, AreaD& d, int& eb, bool launch) {
  SC_REQUIRE(a, "sc_warp_area: null arguments");
  SC_REQUIRE(a->P >= 0 && a->P <= AREA_PMAX, "sc_warp_area: P=%d outside [0, %d]", a->P, AREA_PMAX);
  SC_REQUIRE(a->P > 0 || a->boxes || !launch, "sc_warp_area: nothing to write (P = 0 and no box output)");
  SC_REQUIRE(a->P == 0 || a->out, "sc_warp_area: null output pointer");
  SC_REQUIRE(a->out_h >= 1 && a->out_w >= 1 && a->src_h >= 1 && a->src_w >= 1, "sc_warp_area: bad dims out %d x %d, source %d x %d",
             a->out_h, a->out_w, a->src_h, a->src_w);
  SC_REQUIRE((long long)a->out_h * a->out_w < (1LL << 31), "sc_warp_area: %d x %d output pixels do not fit 31 bits", a->out_h, a->out_w);
  SC_REQUIRE(a->variant >= 0 && a->variant <= SC_WARP_AREA_LANES, "sc_warp_area: variant %d (0 = chosen here, 1 = thread, 2 = lane group)",
             a->variant);
  eb = a->P ? a->elem_bytes : 4;
  const int mode = a->P ? a->mode : SC_WARP_AREA_AVERAGE;
  SC_REQUIRE(mode >= SC_WARP_AREA_AVERAGE && mode <= SC_WARP_AREA_MODE, "sc_warp_area: mode %d (2 = average, 3 = max, 4 = min, 5 = mode)", mode);
  SC_REQUIRE(eb == 4 || eb == 1, "sc_warp_area: element width %d (4 = float32 or 1 = uint8 expected)", eb);
  SC_REQUIRE(mode != SC_WARP_AREA_AVERAGE || eb == 4, "sc_warp_area: average is defined for float32 planes, not %d-byte elements", eb);
  SC_REQUIRE(mode != SC_WARP_AREA_MODE || eb == 1, "sc_warp_area: mode is defined for uint8 planes, not %d-byte elements", eb);
  SC_REQUIRE(a->min_coverage >= 0.0 && a->min_coverage <= 1.0, "sc_warp_area: min_coverage %g outside [0, 1]", a->min_coverage);
  SC_REQUIRE((uintptr_t)a->out % eb == 0 && (uintptr_t)a->coverage % 4 == 0 && (uintptr_t)a->boxes % 8 == 0,
             "sc_warp_area: misaligned output, coverage or box pointer");
  SC_REQUIRE(a->P > 0 || !a->coverage, "sc_warp_area: a coverage output without planes");
  if (int rc = grid_pair_setup(d, "sc_warp_area", a->dst_gt, a->src_inv, a->dst_crs, a->src_crs)) return rc;
  d.H = a->out_h; d.W = a->out_w; d.sh = a->src_h; d.sw = a->src_w; d.P = a->P; d.tiles_x = 0;
  d.min_cov = a->min_coverage;
  d.flip = mode == SC_WARP_AREA_MIN ? 0xFFFFFFFFu : 0u;
  d.out = a->out; d.cov = a->coverage; d.boxes = a->boxes;
  return grid_planes(d, "sc_warp_area", a, eb);
}

}  // namespace

extern "C" int sc_warp_area_variant(const sc_warp_area_args* a) {
  AreaD d;
  int eb;
  const int rc = prepare(a, d, eb, false);
  if (rc) return rc;
  return a->variant ? a->variant : area_variant(d);
}

extern "C" int sc_warp_area(const sc_warp_area_args* a, sc_stream stream) {
  AreaD d;
  int eb;
  const int rc = prepare(a, d, eb, true);
  if (rc) return rc;
  const int variant = a->variant ? a->variant : area_variant(d);
  const bool vec = a->out_w % 4 == 0 && (uintptr_t)a->out % (uintptr_t)(4 * eb) == 0 && (uintptr_t)a->coverage % 16 == 0;
  const int mode = a->P ? a->mode : SC_WARP_AREA_AVERAGE;
  hipStream_t st = (hipStream_t)stream;
  if (mode == SC_WARP_AREA_AVERAGE) launch<uint32_t, K_AVG>(d, variant, vec, st);
  else if (mode == SC_WARP_AREA_MODE) launch<uint8_t, K_MODE>(d, variant, vec, st);
  else if (eb == 4) launch<uint32_t, K_EXT>(d, variant, vec, st);
  else launch<uint8_t, K_EXT>(d, variant, vec, st);
  SC_LAUNCH_OK("sc_warp_area");
  return SC_OK;
}
