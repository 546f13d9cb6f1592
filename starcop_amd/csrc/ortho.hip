// Orthorectification through a geometry look-up table (starcop/models/mag1c_emit.py:86-88: ei.georreference(mag1c_output, ...) and
// the same call on the albedo; the gather itself is restated in the note at :206-221): P planes in sensor geometry are resampled
// onto the GLT's grid in ONE launch,
//   out[p][i][j] = src_p[gy - 1][gx - 1]   if glt_x[i][j] != 0 and glt_y[i][j] != 0      ((gx, gy) = the two GLT words, 1-based;
//                  fill[p]                 otherwise                                       their absolute values with `absolute`)
// so the two GLT words of a pixel are read once, not once per plane.  Pure data movement: elements are copied as 1-, 2-, 4- or
// 8-byte words and the fill values are bit patterns, so NaN payloads and -0.0 survive and the result is bit-equal to the numpy
// gather for every dtype of that width.
//   Mapping: a work-group of 256 threads owns a tile of 16 rows x 256 bytes of one output plane (64 float32 pixels); a thread owns 16
//   bytes of consecutive pixels of one row (V = 16 / width pixels: one 16-byte store per plane, 16-byte GLT loads), so a wave
//   writes four 256-byte runs and reads eight 256-byte-or-longer GLT runs, all whole 128-byte lines.  The tile is two-dimensional
//   because the source side is a gather: a rotated swath maps a 64 x 4 block of output pixels onto a compact patch of the source,
//   while 256 pixels of ONE output row would cross ~256 sin(angle) source rows and use a few elements of each line they touch.
//   When the output width is not a multiple of V (or a pointer is not 16-byte aligned) rows do not start on 16-byte boundaries:
//   the same kernel runs with V = 1 and a tile of 4 rows x 64 pixels (one row per wave).
// GLT entries that point outside the swath (0 < gx <= cols, 0 < gy <= rows does not hold) never reach a load: the pixel gets the
// fill value and the thread adds its count to *oob_count (one atomic per thread that saw any; none on clean data).  A plane may
// cover only the top-left plane_rows x plane_cols of the swath (the network output is cropped to multiples of 32): entries beyond
// it give the fill value and are not counted.  No LDS, no other atomics: repeated calls give identical bits.
#include <limits.h>

#include "sc_common.h"

namespace {

constexpr int ORTHO_PMAX = SC_ORTHO_MAX_PLANES;
constexpr int ORTHO_WG = 256;

struct OrthoD {
  const int32_t* gx;
  const int32_t* gy;
  void* out;
  unsigned long long* oob;
  int H, W, rows, cols, P, absolute, tiles_x;
  const void* src[ORTHO_PMAX];
  long long rs[ORTHO_PMAX], cs[ORTHO_PMAX];      // element strides of a source row / column
  int pr[ORTHO_PMAX], pc[ORTHO_PMAX];            // extent of plane p inside the swath
  unsigned long long fill[ORTHO_PMAX];
};

template <class T, int V>
struct alignas((V * sizeof(T) >= 16) ? 16 : V * sizeof(T)) Pack {
  T v[V];
};

// zero-based swath index of a 1-based GLT word, or 0xFFFFFFFF... (>= any extent) for "no data" / out of range
__device__ __forceinline__ unsigned glt_index(int g, int absolute) {
  const unsigned u = (absolute && g < 0) ? 0u - (unsigned)g : (unsigned)g;
  return u - 1u;
}

// grid.x = tiles_y * tiles_x tiles of TY rows x TX * V pixels
template <class T, int V>
__global__ __launch_bounds__(ORTHO_WG) void k_glt_ortho(OrthoD a) {
  constexpr int TX = V == 1 ? 64 : 16, TY = ORTHO_WG / TX;
  const int by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const long long x0 = ((long long)bx * TX + tx) * V;
  const int y = by * TY + ty;
  if (y >= a.H || x0 >= a.W) return;              // W % V == 0 on the vector path: a thread's V pixels are inside the row or all outside
  const size_t pix = (size_t)y * a.W + (size_t)x0;
  const Pack<int32_t, V> gx = *reinterpret_cast<const Pack<int32_t, V>*>(a.gx + pix);
  const Pack<int32_t, V> gy = *reinterpret_cast<const Pack<int32_t, V>*>(a.gy + pix);
  unsigned sx[V], sy[V];
  unsigned bad = 0;
#pragma unroll
  for (int u = 0; u < V; ++u) {
    const bool data = gx.v[u] != 0 && gy.v[u] != 0;
    const unsigned ux = glt_index(gx.v[u], a.absolute), uy = glt_index(gy.v[u], a.absolute);
    const bool in = data && ux < (unsigned)a.cols && uy < (unsigned)a.rows;
    bad += (data && !in) ? 1u : 0u;
    sx[u] = in ? ux : 0xFFFFFFFFu;
    sy[u] = in ? uy : 0xFFFFFFFFu;
  }
  if (bad && a.oob) atomicAdd(a.oob, (unsigned long long)bad);
  const size_t plane = (size_t)a.H * a.W;
  T* o = static_cast<T*>(a.out) + pix;
  for (int p = 0; p < a.P; ++p) {                 // p is uniform: the plane's descriptor comes in scalar registers
    const T* s = static_cast<const T*>(a.src[p]);
    const long long rs = a.rs[p], cs = a.cs[p];
    const unsigned pr = (unsigned)a.pr[p], pc = (unsigned)a.pc[p];
    const T fill = (T)a.fill[p];
    Pack<T, V> r;
#pragma unroll
    for (int u = 0; u < V; ++u) {
      T v = fill;
      if (sx[u] < pc && sy[u] < pr) v = s[(long long)sy[u] * rs + (long long)sx[u] * cs];
      r.v[u] = v;
    }
    *reinterpret_cast<Pack<T, V>*>(o + (size_t)p * plane) = r;
  }
}

template <class T>
int launch(const OrthoD& d0, bool vec, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  OrthoD d = d0;
  const int tw = vec ? 16 * V : 64, th = vec ? ORTHO_WG / 16 : ORTHO_WG / 64;
  d.tiles_x = (d.W + tw - 1) / tw;
  const long long tiles = (long long)d.tiles_x * ((d.H + th - 1) / th);
  SC_REQUIRE(tiles <= INT_MAX, "sc_glt_ortho: grid too large for one launch");
  if (vec) hipLaunchKernelGGL((k_glt_ortho<T, V>), dim3((unsigned)tiles), dim3(ORTHO_WG), 0, st, d);
  else hipLaunchKernelGGL((k_glt_ortho<T, 1>), dim3((unsigned)tiles), dim3(ORTHO_WG), 0, st, d);
  return SC_OK;
}

}  // namespace

extern "C" int sc_glt_ortho(const sc_ortho_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_glt_ortho: null arguments");
  SC_REQUIRE(a->glt_x && a->glt_y && a->out, "sc_glt_ortho: null pointer");
  SC_REQUIRE(a->out_h >= 1 && a->out_w >= 1 && a->rows >= 1 && a->cols >= 1, "sc_glt_ortho: bad dims out %d x %d, swath %d x %d",
             a->out_h, a->out_w, a->rows, a->cols);
  SC_REQUIRE(a->P >= 1 && a->P <= ORTHO_PMAX, "sc_glt_ortho: P=%d outside [1, %d]", a->P, ORTHO_PMAX);
  const int eb = a->elem_bytes;
  SC_REQUIRE(eb == 1 || eb == 2 || eb == 4 || eb == 8, "sc_glt_ortho: element width %d (1, 2, 4 or 8 bytes expected)", eb);
  SC_REQUIRE((uintptr_t)a->glt_x % 4 == 0 && (uintptr_t)a->glt_y % 4 == 0 && (uintptr_t)a->out % eb == 0,
             "sc_glt_ortho: misaligned GLT or output pointer");
  OrthoD d;
  d.gx = a->glt_x; d.gy = a->glt_y; d.out = a->out; d.oob = (unsigned long long*)a->oob_count;
  d.H = a->out_h; d.W = a->out_w; d.rows = a->rows; d.cols = a->cols; d.P = a->P; d.absolute = a->absolute ? 1 : 0; d.tiles_x = 0;
  for (int p = 0; p < ORTHO_PMAX; ++p) {
    const bool on = p < a->P;
    if (on) {
      SC_REQUIRE_PLANE("sc_glt_ortho", a->src[p], a->row_stride[p], a->col_stride[p], eb, p);
      SC_REQUIRE(a->plane_rows[p] >= 0 && a->plane_rows[p] <= a->rows && a->plane_cols[p] >= 0 && a->plane_cols[p] <= a->cols,
                 "sc_glt_ortho: plane %d extent %d x %d outside the %d x %d swath", p, a->plane_rows[p], a->plane_cols[p], a->rows, a->cols);
    }
    d.src[p] = on ? a->src[p] : nullptr;
    d.rs[p] = on ? a->row_stride[p] : 0;
    d.cs[p] = on ? a->col_stride[p] : 0;
    d.pr[p] = on ? (a->plane_rows[p] ? a->plane_rows[p] : a->rows) : 0;
    d.pc[p] = on ? (a->plane_cols[p] ? a->plane_cols[p] : a->cols) : 0;
    d.fill[p] = on ? a->fill_bits[p] : 0;
  }
  const int V = 16 / eb;
  const bool vec = a->out_w % V == 0 && (uintptr_t)a->out % 16 == 0 && (uintptr_t)a->glt_x % 16 == 0 && (uintptr_t)a->glt_y % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (eb == 1) rc = launch<uint8_t>(d, vec, st);
  else if (eb == 2) rc = launch<uint16_t>(d, vec, st);
  else if (eb == 4) rc = launch<uint32_t>(d, vec, st);
  else rc = launch<uint64_t>(d, vec, st);
  if (rc) return rc;
  SC_LAUNCH_OK("sc_glt_ortho");
  return SC_OK;
}
