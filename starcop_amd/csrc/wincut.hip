// Cutting the sampled windows of a flight line into dense sample tensors (starcop/data/sampling_dataset.py:259-303,
// WindowDataset.__getitem__: read_from_window(window, boundless=True).load(boundless=True) at :266, nodata -> 0 at :269-271, the
// float32 multiply at :285 / :289 and np.clip at :287 / :293): n_win windows of P source planes in ONE launch,
//   out[w][p][i][j] = post_p( plane p holds (r, c) ? src_p[(r - row0_p) * row_stride_p + (c - col0_p) * col_stride_p] : 0 ),
//   (r, c) = (row_off[w] + i, col_off[w] + j),   post_p = fill -> 0, then * scale_p, then clip to [lo_p, hi_p] (each optional).
// Reads are boundless: a window may hang over any edge of the scene, lie outside it or be larger than it; what no plane element
// covers is zero.  Nothing outside a plane's extent is ever dereferenced, whatever the offsets are.
//   Mapping: the output is a dense stream, so the launch is cut along it.  A work-group of 256 threads owns 16 KiB of consecutive
//   output of one (window, plane) pair (1024 16-byte vectors; the pair is uniform, so its descriptor and window offsets come in
//   scalar registers); a thread owns four 16-byte vectors 4 KiB apart, its four loads are independent and issued together.
//   Consecutive lanes hold consecutive vectors of an output row, i.e. one wave-instruction stores 1 KiB contiguously and reads one
//   contiguous run of a source row (or two, where an output row ends inside the wave: rows shorter than 1 KiB).  The source column
//   offset is arbitrary (col_off mod 4 takes every value), so a vector is read as 16 consecutive bytes at element alignment when all
//   of it lies inside the plane on unit column stride, and element by element where it crosses the plane's edge or the plane is a band
//   of a pixel-interleaved cube (col_stride = bands: a strided read is all such a layout allows).
//   When out_w * elem_bytes is not a multiple of 16 (or `out` is not 16-byte aligned) rows do not start on 16-byte boundaries:
//   the same kernel runs with one element per vector.
// No LDS, no atomics, plain vector stores inside `out` only: repeated calls give identical bits.
#include <limits.h>
#include <string.h>

#include <vector>

#include "sc_common.h"

namespace {

constexpr int WCUT_PMAX = SC_WCUT_MAX_PLANES;
constexpr int WCUT_WG = 256;
constexpr int WCUT_PER_THREAD = 4;
constexpr unsigned WCUT_CHUNK = WCUT_WG * WCUT_PER_THREAD;      // vectors per work-group

struct WcutD {
  const int32_t* win;                            // [n_win][2] (row_off, col_off)
  void* out;
  int ow, P;
  unsigned vpr, vpp, chunks;                     // vectors per output row / per output plane, work-groups per plane
  const void* src[WCUT_PMAX];
  long long rs[WCUT_PMAX], cs[WCUT_PMAX];        // element strides of a source row / column
  int r0[WCUT_PMAX], c0[WCUT_PMAX];              // origin of plane p inside the scene
  int nr[WCUT_PMAX], nc[WCUT_PMAX];              // its extent
  unsigned ops[WCUT_PMAX], fill[WCUT_PMAX];
  float scale[WCUT_PMAX], lo[WCUT_PMAX], hi[WCUT_PMAX];
};
static_assert(sizeof(WcutD) <= 4096, "the descriptor travels as a kernel argument");

template <class T, int V>
struct alignas((V * sizeof(T) >= 16) ? 16 : V * sizeof(T)) WPack {
  T v[V];
};

template <class T, bool FOPS>
__device__ __forceinline__ T wcut_post(T v, unsigned ops, unsigned fill, float scale, float lo, float hi) {
  if constexpr (FOPS) {
    float f = __uint_as_float((unsigned)v);
    if ((ops & SC_WCUT_FILL) && f == __uint_as_float(fill)) f = 0.f;      // a NaN fill compares unequal to everything
    if (ops & SC_WCUT_SCALE) f = f * scale;
    if (ops & SC_WCUT_CLIP) {                                             // numpy.clip: NaN fails both comparisons and stays
      f = f < lo ? lo : f;
      f = f > hi ? hi : f;
    }
    return (T)__float_as_uint(f);
  } else {
    return ((ops & SC_WCUT_FILL) && v == (T)fill) ? (T)0 : v;
  }
}

// grid.x = n_win * P * chunks work-groups
template <class T, int V, bool FOPS>
__global__ __launch_bounds__(WCUT_WG) void k_window_cut(WcutD a) {
  const unsigned wp = blockIdx.x / a.chunks, ch = blockIdx.x - wp * a.chunks;
  const unsigned w = wp / (unsigned)a.P, p = wp - w * (unsigned)a.P;
  const long long ro = a.win[2 * (size_t)w], co = a.win[2 * (size_t)w + 1];
  const T* s = static_cast<const T*>(a.src[p]);
  const long long rs = a.rs[p], cs = a.cs[p];
  const long long r0 = a.r0[p], c0 = a.c0[p], nr = a.nr[p], nc = a.nc[p];
  const unsigned ops = a.ops[p], fill = a.fill[p];
  const float scale = a.scale[p], lo = a.lo[p], hi = a.hi[p];
  T* o = static_cast<T*>(a.out) + (size_t)wp * a.vpp * V;
#pragma unroll
  for (int k = 0; k < WCUT_PER_THREAD; ++k) {
    const unsigned t = ch * WCUT_CHUNK + k * WCUT_WG + threadIdx.x;
    if (t < a.vpp) {
      const unsigned i = t / a.vpr, jv = t - i * a.vpr;
      const long long rr = ro + i - r0;
      const long long cc = co + (long long)jv * V - c0;
      const bool row_in = rr >= 0 && rr < nr;
      WPack<T, V> r;
      if (row_in && cc >= 0 && cc + V <= nc) {
        const T* q = s + rr * rs + cc * cs;
        if (V > 1 && cs == 1) {
          // the lanes of a row share the residue of their address mod 16: one 16-byte load where it is 0, else an element-aligned
          // read of the same 16 bytes (global_load_dword + global_load_dwordx3 at 4-byte elements)
          if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) r = *reinterpret_cast<const WPack<T, V>*>(q);
          else __builtin_memcpy(&r, q, sizeof(r));
        } else {
#pragma unroll
          for (int u = 0; u < V; ++u) r.v[u] = q[u * cs];
        }
      } else {
#pragma unroll
        for (int u = 0; u < V; ++u) {
          const long long cu = cc + u;
          T v = 0;
          if (row_in && cu >= 0 && cu < nc) v = s[rr * rs + cu * cs];
          r.v[u] = v;
        }
      }
#pragma unroll
      for (int u = 0; u < V; ++u) r.v[u] = wcut_post<T, FOPS>(r.v[u], ops, fill, scale, lo, hi);
      *reinterpret_cast<WPack<T, V>*>(o + (size_t)t * V) = r;
    }
  }
}

template <class T, bool FOPS>
int launch(WcutD d, int oh, int n_win, bool vec, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  const int v = vec ? V : 1;
  d.vpr = (unsigned)(d.ow / v);
  d.vpp = d.vpr * (unsigned)oh;
  d.chunks = (d.vpp + WCUT_CHUNK - 1) / WCUT_CHUNK;
  const long long blocks = (long long)n_win * d.P * d.chunks;
  SC_REQUIRE(blocks <= INT_MAX, "sc_window_cut: grid of %lld work-groups is too large for one launch", blocks);
  if (vec) hipLaunchKernelGGL((k_window_cut<T, V, FOPS>), dim3((unsigned)blocks), dim3(WCUT_WG), 0, st, d);
  else hipLaunchKernelGGL((k_window_cut<T, 1, FOPS>), dim3((unsigned)blocks), dim3(WCUT_WG), 0, st, d);
  return SC_OK;
}

}  // namespace

extern "C" int sc_window_cut(const sc_wcut_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_window_cut: null arguments");
  SC_REQUIRE(a->win_off && a->win_off_host && a->out, "sc_window_cut: null pointer");
  SC_REQUIRE(a->scene_rows >= 1 && a->scene_cols >= 1, "sc_window_cut: bad scene dims %d x %d", a->scene_rows, a->scene_cols);
  SC_REQUIRE(a->out_h >= 1 && a->out_w >= 1 && (long long)a->out_h * a->out_w < (1ll << 31), "sc_window_cut: bad window size %d x %d",
             a->out_h, a->out_w);
  SC_REQUIRE(a->P >= 1 && a->P <= WCUT_PMAX, "sc_window_cut: P=%d outside [1, %d]", a->P, WCUT_PMAX);
  SC_REQUIRE(a->n_win >= 1 && a->n_win <= (1 << 20), "sc_window_cut: n_win=%d outside [1, 2^20]", a->n_win);
  const int eb = a->elem_bytes;
  SC_REQUIRE(eb == 1 || eb == 2 || eb == 4, "sc_window_cut: element width %d (1, 2 or 4 bytes expected)", eb);
  SC_REQUIRE((uintptr_t)a->out % eb == 0 && (uintptr_t)a->win_off % 4 == 0, "sc_window_cut: misaligned output or window pointer");
  WcutD d;
  d.win = a->win_off; d.out = a->out; d.ow = a->out_w; d.P = a->P; d.vpr = d.vpp = d.chunks = 0;
  bool fops = false;
  for (int p = 0; p < WCUT_PMAX; ++p) {
    const bool on = p < a->P;
    if (on) {
      SC_REQUIRE_PLANE("sc_window_cut", a->src[p], a->row_stride[p], a->col_stride[p], eb, p);
      SC_REQUIRE(a->rows[p] >= 1 && a->cols[p] >= 1 && a->row0[p] >= 0 && a->col0[p] >= 0 &&
                     (long long)a->row0[p] + a->rows[p] <= a->scene_rows && (long long)a->col0[p] + a->cols[p] <= a->scene_cols,
                 "sc_window_cut: plane %d (%d x %d at row %d, col %d) is not inside the %d x %d scene", p, a->rows[p], a->cols[p],
                 a->row0[p], a->col0[p], a->scene_rows, a->scene_cols);
      SC_REQUIRE((a->ops[p] & ~(uint32_t)(SC_WCUT_FILL | SC_WCUT_SCALE | SC_WCUT_CLIP)) == 0, "sc_window_cut: unknown ops bits 0x%x of plane %d",
                 a->ops[p], p);
      if (a->ops[p] & (SC_WCUT_SCALE | SC_WCUT_CLIP)) {
        SC_REQUIRE(eb == 4, "sc_window_cut: scale / clip of plane %d need 4-byte (float32) elements, got %d-byte ones", p, eb);
        fops = true;
      }
      if (a->ops[p] & SC_WCUT_CLIP)
        SC_REQUIRE(a->clip_lo[p] <= a->clip_hi[p], "sc_window_cut: clip bounds of plane %d are not ordered (or NaN)", p);
      if ((a->ops[p] & SC_WCUT_FILL) && eb < 4)
        SC_REQUIRE((a->fill_bits[p] >> (8 * eb)) == 0, "sc_window_cut: fill pattern 0x%x of plane %d is wider than %d bytes", a->fill_bits[p], p, eb);
    }
    d.src[p] = on ? a->src[p] : nullptr;
    d.rs[p] = on ? a->row_stride[p] : 0;
    d.cs[p] = on ? a->col_stride[p] : 0;
    d.r0[p] = on ? a->row0[p] : 0;
    d.c0[p] = on ? a->col0[p] : 0;
    d.nr[p] = on ? a->rows[p] : 0;
    d.nc[p] = on ? a->cols[p] : 0;
    d.ops[p] = on ? a->ops[p] : 0;
    d.fill[p] = on ? a->fill_bits[p] : 0;
    d.scale[p] = on ? a->scale[p] : 1.f;
    d.lo[p] = on ? a->clip_lo[p] : 0.f;
    d.hi[p] = on ? a->clip_hi[p] : 0.f;
  }
  for (int i = 0; i < a->n_win; ++i) {
    const int32_t* q = a->win_off_host + (size_t)i * 2;
    SC_REQUIRE((long long)q[0] + a->out_h <= INT_MAX && (long long)q[1] + a->out_w <= INT_MAX,
               "sc_window_cut: window %d (row %d, col %d, %d x %d) leaves the int32 range", i, q[0], q[1], a->out_h, a->out_w);
  }
  hipStream_t st = (hipStream_t)stream;
  {
    // the device copy of the table is what the kernel walks: it must be the table that was just checked
    std::vector<int32_t> dev((size_t)a->n_win * 2);
    const size_t bytes = dev.size() * sizeof(int32_t);
    if (hipMemcpyAsync(dev.data(), a->win_off, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      (void)hipGetLastError();
      sc_set_error("sc_window_cut: reading back the device window table failed");
      return SC_ERR_LAUNCH;
    }
    SC_REQUIRE(memcmp(dev.data(), a->win_off_host, bytes) == 0, "sc_window_cut: the host and device window tables differ");
  }
  const int V = 16 / eb;
  const bool vec = a->out_w % V == 0 && (uintptr_t)a->out % 16 == 0;
  int rc;
  if (eb == 1) rc = launch<uint8_t, false>(d, a->out_h, a->n_win, vec, st);
  else if (eb == 2) rc = launch<uint16_t, false>(d, a->out_h, a->n_win, vec, st);
  else if (fops) rc = launch<uint32_t, true>(d, a->out_h, a->n_win, vec, st);
  else rc = launch<uint32_t, false>(d, a->out_h, a->n_win, vec, st);
  if (rc) return rc;
  SC_LAUNCH_OK("sc_window_cut");
  return SC_OK;
}
