// Reprojection of rasters between grids (the warp): for every pixel (r, c) of a destination grid
//   1. world coordinates of the pixel centre (c + 0.5, r + 0.5) through the destination's 6-term affine geotransform,
//   2. destination CRS -> source CRS: nothing (same CRS), WGS-84 UTM -> longitude / latitude, longitude / latitude -> UTM, or zone A ->
//      zone B through longitude / latitude.  Transverse Mercator is the Krueger series in the third flattening n to order n^6 (Karney
//      2011, "Transverse Mercator with an accuracy of a few nanometers", eq. 35 / 36: the alpha and beta coefficients), summed with a
//      complex Clenshaw recurrence; the conformal latitude is inverted with a FIXED number of Newton steps (no data-dependent loop),
//   3. source pixel coordinates (u, v) through the inverse of the source's affine (inverted on the host in float64),
//   4. sampling of P planes: `nearest` copies element (floor(v), floor(u)) as a 1-, 2-, 4- or 8-byte word (bit-equal to a numpy gather
//      for every dtype); `bilinear` (float32) weighs the four pixels around (u - 0.5, v - 0.5) in fp64, leaves out samples that lie
//      outside the raster, are NaN or carry the plane's no-data bit pattern, divides by the weight of those that count and rounds once.
//   Footprint rule of both modes: the pixel gets the plane's no-data when (u, v) is outside [0, W) x [0, H), when the projection has
//   no finite result or leaves the 30 degrees around the zone's central meridian; `bilinear` also when the NEAREST source pixel does
//   not count -- so bilinear and nearest of one plane have the same valid pixels and data never bleeds into fill.
// everything in fp64, all of it once per pixel and not once per plane (as sc_glt_ortho reads its GLT words once).
//   Mapping: the two-dimensional tiles of ortho.hip, because the source side is a gather: a work-group of 256 threads owns 16 rows x
//   64 pixels, a thread 4 consecutive pixels of a row (one 16-byte store per float32 plane; 2 pixels = 16 bytes for 8-byte elements).
//   A thread never owns more than 4 pixels: each costs two fp64 series with ~20 transcendental calls, and 16 unrolled copies of that
//   for one-byte elements would not fit the instruction cache -- a uint8 mask is stored as 4-byte words instead.  When the width is
//   not a multiple of the vector (or a pointer is not aligned to the store) the same kernel runs with one pixel per thread and tiles
//   of 4 rows x 64 pixels.  No LDS; the only atomic is the optional count of pixels outside the source: two calls give the same bytes.
#include <limits.h>
#include <math.h>

#include <cmath>

#include "sc_common.h"
#include "sc_warp.h"

namespace {

constexpr int WARP_PMAX = SC_WARP_MAX_PLANES;
constexpr int WARP_WG = 256;

struct WarpD {
  double gt[6], inv[6];
  Krueger k;
  double dst_lon0, dst_fn, src_lon0, src_fn;     // central meridian (degrees) and false northing of a UTM side
  int route;                                     // bit 0: destination is UTM (inverse first), bit 1: source is UTM (forward after)
  int H, W, sh, sw, P, tiles_x;
  int unbounded;                                 // coordinates only: (u, v) outside the source raster are kept
  void* out;
  double* coords;
  unsigned long long* oob;
  const void* src[WARP_PMAX];
  long long rs[WARP_PMAX], cs[WARP_PMAX];
  unsigned long long nod[WARP_PMAX];
};

// source pixel coordinates of the centre of destination pixel (r, c); NaN when the point is outside the source
__device__ __forceinline__ bool source_uv(const WarpD& a, int r, long long c, double& u, double& v) {
  bool ok = grid_uv(a, (double)c + 0.5, (double)r + 0.5, u, v);
  const bool inside = u >= 0.0 && u < (double)a.sw && v >= 0.0 && v < (double)a.sh;      // false for NaN and infinities
  ok = ok && (inside || (a.unbounded && fabs(u) < INFINITY && fabs(v) < INFINITY));
  if (!ok) u = v = __builtin_nan("");
  return ok;
}

// grid.x = tiles_y * tiles_x tiles of TY rows x TX * V pixels.  BIL: bilinear (T = uint32_t, the bits of a float32)
template <class T, int V, bool BIL>
__global__ __launch_bounds__(WARP_WG) void k_warp(WarpD a) {
  constexpr int TX = V == 1 ? 64 : 16, TY = WARP_WG / TX;
  const int by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const long long x0 = ((long long)bx * TX + tx) * V;
  const int y = by * TY + ty;
  if (y >= a.H || x0 >= a.W) return;              // W % V == 0 on the vector path: a thread's V pixels are inside the row or all outside
  const size_t pix = (size_t)y * a.W + (size_t)x0;
  const size_t plane = (size_t)a.H * a.W;
  double u[V], v[V];
  bool in[V];
  unsigned bad = 0;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    in[e] = source_uv(a, y, x0 + e, u[e], v[e]);
    bad += in[e] ? 0u : 1u;
  }
  if (bad && a.oob) atomicAdd(a.oob, (unsigned long long)bad);
  if (a.coords) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      a.coords[pix + e] = u[e];
      a.coords[plane + pix + e] = v[e];
    }
  }
  if (a.P == 0) return;
  T* o = static_cast<T*>(a.out) + pix;
  for (int p = 0; p < a.P; ++p) {                 // p is uniform: the plane's descriptor comes in scalar registers
    const T* s = static_cast<const T*>(a.src[p]);
    const long long rs = a.rs[p], cs = a.cs[p];
    const T nod = (T)a.nod[p];
    Pack<T, V> r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = sample<T, BIL>(s, rs, cs, nod, a.sh, a.sw, u[e], v[e], in[e]);
    *reinterpret_cast<Pack<T, V>*>(o + (size_t)p * plane) = r;
  }
}

template <class T, int V, bool BIL>
int launch(const WarpD& d0, bool vec, hipStream_t st) {
  WarpD d = d0;
  const int tw = vec ? 16 * V : 64, th = vec ? WARP_WG / 16 : WARP_WG / 64;
  d.tiles_x = (d.W + tw - 1) / tw;
  const long long tiles = (long long)d.tiles_x * ((d.H + th - 1) / th);
  SC_REQUIRE(tiles <= INT_MAX, "sc_warp: grid too large for one launch");
  if (vec) hipLaunchKernelGGL((k_warp<T, V, BIL>), dim3((unsigned)tiles), dim3(WARP_WG), 0, st, d);
  else hipLaunchKernelGGL((k_warp<T, 1, BIL>), dim3((unsigned)tiles), dim3(WARP_WG), 0, st, d);
  return SC_OK;
}

}  // namespace

extern "C" int sc_warp(const sc_warp_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_warp: null arguments");
  SC_REQUIRE(a->P >= 0 && a->P <= WARP_PMAX, "sc_warp: P=%d outside [0, %d]", a->P, WARP_PMAX);
  SC_REQUIRE(a->P > 0 || a->coords, "sc_warp: nothing to write (P = 0 and no coordinate output)");
  SC_REQUIRE(a->P == 0 || a->out, "sc_warp: null output pointer");
  SC_REQUIRE(a->out_h >= 1 && a->out_w >= 1 && a->src_h >= 1 && a->src_w >= 1, "sc_warp: bad dims out %d x %d, source %d x %d",
             a->out_h, a->out_w, a->src_h, a->src_w);
  SC_REQUIRE((long long)a->out_h * a->out_w < (1LL << 31), "sc_warp: %d x %d output pixels do not fit 31 bits", a->out_h, a->out_w);
  const int eb = a->P ? a->elem_bytes : 4;
  SC_REQUIRE(eb == 1 || eb == 2 || eb == 4 || eb == 8, "sc_warp: element width %d (1, 2, 4 or 8 bytes expected)", eb);
  SC_REQUIRE(a->resampling == SC_WARP_NEAREST || a->resampling == SC_WARP_BILINEAR, "sc_warp: resampling %d (0 = nearest, 1 = bilinear)",
             a->resampling);
  SC_REQUIRE((a->flags & ~SC_WARP_UNBOUNDED) == 0 && (a->flags == 0 || a->P == 0),
             "sc_warp: flags %d (SC_WARP_UNBOUNDED, and only with P = 0: planes are never read outside the raster)", a->flags);
  const bool bil = a->P > 0 && a->resampling == SC_WARP_BILINEAR;
  SC_REQUIRE(!bil || eb == 4, "sc_warp: bilinear resampling is defined for float32 planes, not %d-byte elements", eb);
  SC_REQUIRE((uintptr_t)a->out % eb == 0 && (uintptr_t)a->coords % 8 == 0 && (uintptr_t)a->oob_count % 8 == 0,
             "sc_warp: misaligned output, coordinate or counter pointer");
  WarpD d;
  if (int rc = grid_pair_setup(d, "sc_warp", a->dst_gt, a->src_inv, a->dst_crs, a->src_crs)) return rc;
  d.H = a->out_h; d.W = a->out_w; d.sh = a->src_h; d.sw = a->src_w; d.P = a->P; d.tiles_x = 0;
  d.unbounded = a->flags & SC_WARP_UNBOUNDED;
  d.out = a->out; d.coords = a->coords; d.oob = (unsigned long long*)a->oob_count;
  if (int rc = grid_planes(d, "sc_warp", a, eb)) return rc;
  const int V = eb == 8 ? 2 : 4;
  const uintptr_t store = (uintptr_t)(V * eb < 16 ? V * eb : 16);
  const bool vec = a->out_w % V == 0 && (uintptr_t)a->out % store == 0;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (bil) rc = launch<uint32_t, 4, true>(d, vec, st);
  else if (eb == 1) rc = launch<uint8_t, 4, false>(d, vec, st);
  else if (eb == 2) rc = launch<uint16_t, 4, false>(d, vec, st);
  else if (eb == 4) rc = launch<uint32_t, 4, false>(d, vec, st);
  else rc = launch<uint64_t, 2, false>(d, vec, st);
  if (rc) return rc;
  SC_LAUNCH_OK("sc_warp");
  return SC_OK;
}
