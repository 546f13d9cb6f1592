// Whole-scene cloud masking (starcop/sentinel2/models.py:27-52, 80-89: padded_predict reflect-pads the scene to a multiple of 32 and
// runs it as one image).  sc_scene_gather cuts n equally shaped windows out of the VIRTUAL reflect-padded scene and converts them to
// float32 in the same pass:
//   out[i][c][y][x] = (float) src[c][refl(row_off[i] + y - pad_top, H)][refl(col_off[i] + x - pad_left, W)]   [ * scale ]
//   refl(t, n) = t < 0 ? -t : (t >= n ? 2 (n - 1) - t : t)            (numpy "reflect"; one reflection: pads < n)
// The padded scene is never stored and a uint16 scene stays uint16 in memory; the source is read in place through element strides.
//   Mapping (that of sc_window_cut): the output is a dense stream, cut into 16 KiB pieces of one (window, channel) plane per
//   work-group of 256 threads; a thread owns four 16-byte vectors 4 KiB apart, consecutive lanes hold consecutive vectors of an output
//   row, so one wave-instruction stores 1 KiB contiguously and reads one contiguous run of a source row.  The four source elements of
//   a vector come in one load (8 bytes of uint16, 16 bytes of float32) when they are contiguous (unit column stride), inside the image
//   and aligned to that load; element by element on the reflected fringes, at unaligned columns and at non-unit column strides.
//   Every address is formed in 64 bits.  After the reflection the coordinate is clamped into the image, so whatever the device table
//   holds nothing outside the source is dereferenced; the host copy of the table is what the argument checks read.
// No LDS, no atomics, plain stores inside `out` only: repeated calls give identical bits.
#include <limits.h>

#include "sc_common.h"
#include "sc_scene.h"

namespace {

constexpr int SG_WG = 256;
constexpr int SG_PER_THREAD = 4;
constexpr unsigned SG_CHUNK = SG_WG * SG_PER_THREAD;      // 16-byte output vectors per work-group

struct SceneD {
  const void* src;
  const sc_scene_win* win;
  float* out;
  long long cs, rs, xs;                          // element strides of channel, row, column
  int C, H, W, pad_top, pad_left;
  unsigned vpr, vpp, chunks;                     // vectors per output row / per output plane, work-groups per plane
  float scale;
};

__device__ __forceinline__ long long sg_refl(long long t, long long n) {
  t = t < 0 ? -t : (t >= n ? 2 * (n - 1) - t : t);
  return t < 0 ? 0 : (t >= n ? n - 1 : t);        // (no effect on a checked table)
}

template <class T>
struct alignas(4 * sizeof(T)) SgPack {
  T v[4];
};

// grid.x = n * C * chunks work-groups
template <class T, bool SCALE>
__global__ __launch_bounds__(SG_WG) void k_scene_gather(const SceneD a) {
  const unsigned wc = blockIdx.x / a.chunks, ch = blockIdx.x - wc * a.chunks;
  const unsigned w = wc / (unsigned)a.C, c = wc - w * (unsigned)a.C;
  const long long ro = (long long)a.win[w].row_off - a.pad_top, co = (long long)a.win[w].col_off - a.pad_left;
  const T* s = static_cast<const T*>(a.src) + (long long)c * a.cs;
  float* o = a.out + (size_t)wc * a.vpp * 4;
  const long long H = a.H, W = a.W, xs = a.xs;
#pragma unroll
  for (int k = 0; k < SG_PER_THREAD; ++k) {
    const unsigned t = ch * SG_CHUNK + k * SG_WG + threadIdx.x;
    if (t < a.vpp) {
      const unsigned i = t / a.vpr, jv = t - i * a.vpr;
      const T* row = s + sg_refl(ro + i, H) * a.rs;
      const long long x0 = co + 4ll * jv;
      SgPack<T> r;
      if (xs == 1 && x0 >= 0 && x0 + 4 <= W && (reinterpret_cast<uintptr_t>(row + x0) & (sizeof(r) - 1)) == 0) {
        r = *reinterpret_cast<const SgPack<T>*>(row + x0);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) r.v[u] = row[sg_refl(x0 + u, W) * xs];
      }
      float4 f = make_float4((float)r.v[0], (float)r.v[1], (float)r.v[2], (float)r.v[3]);
      if (SCALE) { f.x *= a.scale; f.y *= a.scale; f.z *= a.scale; f.w *= a.scale; }
      *reinterpret_cast<float4*>(o + (size_t)t * 4) = f;
    }
  }
}

// ---- sc_scene_gather_planes: the same mapping for P float32 planes with a base pointer, strides and a fill / scale / clip operation
// each (the network input of the plume model cut straight out of the products of a flight line).  The (window, plane) pair of a
// work-group is uniform, so its descriptor comes out of the kernel argument in scalar registers.  Elements travel as bit patterns:
// a plane without ops is pure data movement.
constexpr int SP_PMAX = SC_SCENE_MAX_PLANES;
typedef uint32_t sp_u32x4 __attribute__((ext_vector_type(4)));

struct PlanesD {
  const sc_scene_win* win;
  float* out;
  int P, H, W, pad_top, pad_left;
  unsigned vpr, vpp, chunks;
  const uint32_t* src[SP_PMAX];
  long long rs[SP_PMAX], xs[SP_PMAX];
  unsigned ops[SP_PMAX], fill[SP_PMAX];
  float scale[SP_PMAX], lo[SP_PMAX], hi[SP_PMAX];
};

__device__ __forceinline__ uint32_t sp_post(uint32_t b, unsigned ops, unsigned fill, float scale, float lo, float hi) {
  if (ops == 0) return b;
  float f = __uint_as_float(b);
  if ((ops & SC_WCUT_FILL) && b == fill) f = 0.f;
  else if (ops & SC_WCUT_SCALE) f = f * scale;
  if (ops & SC_WCUT_CLIP) {                                               // numpy.clip: NaN fails both comparisons and stays
    f = f < lo ? lo : f;
    f = f > hi ? hi : f;
  }
  return __float_as_uint(f);
}

// the work-group's share of one (window, plane) pair.  UNIT: the plane has unit column stride, so a vector whose four sources lie
// inside the image at a 16-byte aligned address comes in one 16-byte load (a native vector type: a struct-typed 16-byte load is split
// into its members before the two branches are merged, and then stays four 4-byte loads).  Otherwise -- and on the reflected fringes
// and at unaligned columns of a UNIT plane -- element loads.  Every load of the thread's four vectors is requested before the first
// is used; the strided planes get a body without the vector branch, so nothing orders their sixteen element loads.
template <bool UNIT>
__device__ __forceinline__ void sp_gather_body(const PlanesD& a, const uint32_t* s, float* o, unsigned ch, long long ro, long long co,
                                               long long rs, long long xs, unsigned ops, unsigned fill, float scale, float lo, float hi) {
  const long long H = a.H, W = a.W;
  sp_u32x4 r[SG_PER_THREAD];
#pragma unroll
  for (int k = 0; k < SG_PER_THREAD; ++k) {
    const unsigned t = ch * SG_CHUNK + k * SG_WG + threadIdx.x;
    const unsigned tc = t < a.vpp ? t : 0;
    const unsigned i = tc / a.vpr, jv = tc - i * a.vpr;
    const uint32_t* row = s + sg_refl(ro + i, H) * rs;
    const long long x0 = co + 4ll * jv;
    if (UNIT && x0 >= 0 && x0 + 4 <= W && (reinterpret_cast<uintptr_t>(row + x0) & 15) == 0) {
      r[k] = *reinterpret_cast<const sp_u32x4*>(row + x0);
    } else {
      r[k].x = row[sg_refl(x0, W) * xs]; r[k].y = row[sg_refl(x0 + 1, W) * xs];
      r[k].z = row[sg_refl(x0 + 2, W) * xs]; r[k].w = row[sg_refl(x0 + 3, W) * xs];
    }
  }
#pragma unroll
  for (int k = 0; k < SG_PER_THREAD; ++k) {
    const unsigned t = ch * SG_CHUNK + k * SG_WG + threadIdx.x;
    if (t < a.vpp) {
      sp_u32x4 v;
      v.x = sp_post(r[k].x, ops, fill, scale, lo, hi); v.y = sp_post(r[k].y, ops, fill, scale, lo, hi);
      v.z = sp_post(r[k].z, ops, fill, scale, lo, hi); v.w = sp_post(r[k].w, ops, fill, scale, lo, hi);
      *reinterpret_cast<sp_u32x4*>(o + (size_t)t * 4) = v;
    }
  }
}

// grid.x = n * P * chunks work-groups
__global__ __launch_bounds__(SG_WG) void k_scene_gather_planes(const PlanesD a) {
  const unsigned wp = blockIdx.x / a.chunks, ch = blockIdx.x - wp * a.chunks;
  const unsigned w = wp / (unsigned)a.P, p = wp - w * (unsigned)a.P;
  const long long ro = (long long)a.win[w].row_off - a.pad_top, co = (long long)a.win[w].col_off - a.pad_left;
  float* o = a.out + (size_t)wp * a.vpp * 4;
  if (a.xs[p] == 1) sp_gather_body<true>(a, a.src[p], o, ch, ro, co, a.rs[p], 1, a.ops[p], a.fill[p], a.scale[p], a.lo[p], a.hi[p]);
  else sp_gather_body<false>(a, a.src[p], o, ch, ro, co, a.rs[p], a.xs[p], a.ops[p], a.fill[p], a.scale[p], a.lo[p], a.hi[p]);
}

// ---- sc_scene_core_counts: grid (row bands, n); a work-group walks rows blockIdx.x, blockIdx.x + gridDim.x, ... of window
// blockIdx.y's core destination rectangle, a thread four adjacent columns at a time (one 16-byte load where they are contiguous
// and aligned).  Integer partial sums: wave butterfly, LDS, one integer atomic per work-group.  Coordinates are clamped into the
// plane for the address and pixels outside it are not counted, whatever the device table holds.
constexpr int CC_WG = 256;

__global__ __launch_bounds__(CC_WG) void k_scene_core_counts(const uint32_t* __restrict__ plane, long long rs, long long xs, int H, int W,
                                                             unsigned fill, const sc_scene_win* __restrict__ win, int* __restrict__ counts) {
  __shared__ int s_cnt[CC_WG / 64];
  const sc_scene_win q = win[blockIdx.y];
  const long long nr = (long long)q.core_y1 - q.core_y0, nc = (long long)q.core_x1 - q.core_x0;
  int cnt = 0;
  if (nr > 0 && nc > 0) {
    for (long long i = blockIdx.x; i < nr; i += gridDim.x) {
      const long long r = (long long)q.dst_row + i;
      if (r < 0 || r >= H) continue;
      const uint32_t* row = plane + r * rs;
      for (long long j = 4ll * threadIdx.x; j < nc; j += 4ll * CC_WG) {
        const long long c = (long long)q.dst_col + j;
        if (xs == 1 && c >= 0 && c + 4 <= W && j + 4 <= nc && (reinterpret_cast<uintptr_t>(row + c) & 15) == 0) {
          const SgPack<uint32_t> v = *reinterpret_cast<const SgPack<uint32_t>*>(row + c);
#pragma unroll
          for (int u = 0; u < 4; ++u) cnt += v.v[u] != fill;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (j + u < nc && c + u >= 0 && c + u < W) cnt += row[(c + u) * xs] != fill;
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int v = 0; v < CC_WG / 64; ++v) t += s_cnt[v];
    if (t) atomicAdd(&counts[blockIdx.y], t);
  }
}

}  // namespace

extern "C" int sc_scene_gather_planes(const sc_scene_planes_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_scene_gather_planes: null arguments");
  SC_REQUIRE(a->out && a->win && a->win_host, "sc_scene_gather_planes: null pointer");
  SC_REQUIRE(a->P >= 1 && a->P <= SP_PMAX, "sc_scene_gather_planes: P=%d outside [1, %d]", a->P, SP_PMAX);
  SC_REQUIRE(a->H >= 1 && a->W >= 1, "sc_scene_gather_planes: bad scene dims %d x %d", a->H, a->W);
  if (int e = sc_scene_check_gather("sc_scene_gather_planes", a->H, a->W, a->pad_top, a->pad_left, a->n, a->win_h, a->win_w, a->out, a->win, a->win_host))
    return e;
  PlanesD d;
  for (int p = 0; p < SP_PMAX; ++p) {
    const bool on = p < a->P;
    if (on) {
      SC_REQUIRE_PLANE("sc_scene_gather_planes", a->src[p], a->row_stride[p], a->col_stride[p], 4, p);
      SC_REQUIRE((a->ops[p] & ~(uint32_t)(SC_WCUT_FILL | SC_WCUT_SCALE | SC_WCUT_CLIP)) == 0,
                 "sc_scene_gather_planes: unknown ops bits 0x%x of plane %d", a->ops[p], p);
      if (a->ops[p] & SC_WCUT_SCALE) SC_REQUIRE(a->scale[p] == a->scale[p], "sc_scene_gather_planes: scale of plane %d is NaN", p);
      if (a->ops[p] & SC_WCUT_CLIP)
        SC_REQUIRE(a->clip_lo[p] <= a->clip_hi[p], "sc_scene_gather_planes: clip bounds of plane %d are not ordered (or NaN)", p);
    }
    d.src[p] = on ? reinterpret_cast<const uint32_t*>(a->src[p]) : nullptr;
    d.rs[p] = on ? a->row_stride[p] : 0;
    d.xs[p] = on ? a->col_stride[p] : 0;
    d.ops[p] = on ? a->ops[p] : 0;
    d.fill[p] = on ? a->fill_bits[p] : 0;
    d.scale[p] = on ? a->scale[p] : 1.f;
    d.lo[p] = on ? a->clip_lo[p] : 0.f;
    d.hi[p] = on ? a->clip_hi[p] : 0.f;
  }
  d.win = a->win; d.out = a->out;
  d.P = a->P; d.H = a->H; d.W = a->W; d.pad_top = a->pad_top; d.pad_left = a->pad_left;
  d.vpr = (unsigned)(a->win_w / 4);
  d.vpp = d.vpr * (unsigned)a->win_h;
  d.chunks = (d.vpp + SG_CHUNK - 1) / SG_CHUNK;
  const long long blocks = (long long)a->n * a->P * d.chunks;
  SC_REQUIRE(blocks <= INT_MAX, "sc_scene_gather_planes: grid of %lld work-groups is too large for one launch", blocks);
  hipLaunchKernelGGL(k_scene_gather_planes, dim3((unsigned)blocks), dim3(SG_WG), 0, (hipStream_t)stream, d);
  SC_LAUNCH_OK("sc_scene_gather_planes");
  return SC_OK;
}

extern "C" int sc_scene_core_counts(const float* plane, int64_t row_stride, int64_t col_stride, int H, int W, uint32_t fill_bits,
                                    const sc_scene_win* win, const sc_scene_win* win_host, int n, int32_t* counts, sc_stream stream) {
  SC_REQUIRE(plane && win && win_host && counts, "sc_scene_core_counts: null pointer");
  SC_REQUIRE(H >= 1 && W >= 1, "sc_scene_core_counts: bad plane dims %d x %d", H, W);
  SC_REQUIRE(row_stride >= 0 && col_stride >= 0, "sc_scene_core_counts: negative stride");
  SC_REQUIRE(n >= 1 && n <= 65535, "sc_scene_core_counts: n=%d outside [1, 65535]", n);
  SC_REQUIRE((uintptr_t)plane % 4 == 0 && (uintptr_t)win % 4 == 0 && (uintptr_t)counts % 4 == 0, "sc_scene_core_counts: misaligned pointer");
  long long max_rows = 0;
  for (int i = 0; i < n; ++i) {
    const sc_scene_win& q = win_host[i];
    if (q.core_y1 <= q.core_y0 || q.core_x1 <= q.core_x0) continue;      // empty core: 0
    const long long nr = (long long)q.core_y1 - q.core_y0, nc = (long long)q.core_x1 - q.core_x0;
    SC_REQUIRE(q.dst_row >= 0 && q.dst_row + nr <= H && q.dst_col >= 0 && q.dst_col + nc <= W && nr * nc <= INT_MAX,
               "sc_scene_core_counts: core %d (%lld x %lld at row %d, column %d) does not fit the %d x %d plane", i, nr, nc, q.dst_row,
               q.dst_col, H, W);
    max_rows = nr > max_rows ? nr : max_rows;
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess) {
    (void)hipGetLastError();
    sc_set_error("sc_scene_core_counts: memset failed");
    return SC_ERR_LAUNCH;
  }
  if (max_rows == 0) return SC_OK;
  const unsigned bands = (unsigned)(max_rows < 64 ? max_rows : 64);
  hipLaunchKernelGGL(k_scene_core_counts, dim3(bands, (unsigned)n), dim3(CC_WG), 0, st, reinterpret_cast<const uint32_t*>(plane),
                     (long long)row_stride, (long long)col_stride, H, W, (unsigned)fill_bits, win, counts);
  SC_LAUNCH_OK("sc_scene_core_counts");
  return SC_OK;
}

extern "C" int sc_scene_gather(const sc_scene_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_scene_gather: null arguments");
  SC_REQUIRE(a->src && a->out && a->win && a->win_host, "sc_scene_gather: null pointer");
  SC_REQUIRE(a->elem_bytes == 2 || a->elem_bytes == 4, "sc_scene_gather: element width %d (2 = uint16 or 4 = float32 expected)", a->elem_bytes);
  SC_REQUIRE(a->C >= 1 && a->H >= 1 && a->W >= 1, "sc_scene_gather: bad scene dims %d x %d x %d", a->C, a->H, a->W);
  SC_REQUIRE(a->chan_stride >= 0 && a->row_stride >= 0 && a->col_stride >= 0, "sc_scene_gather: negative stride");
  SC_REQUIRE((uintptr_t)a->src % a->elem_bytes == 0, "sc_scene_gather: the source is not aligned to its %d-byte elements", a->elem_bytes);
  SC_REQUIRE(a->scale == a->scale, "sc_scene_gather: scale is NaN");
  if (int e = sc_scene_check_gather("sc_scene_gather", a->H, a->W, a->pad_top, a->pad_left, a->n, a->win_h, a->win_w, a->out, a->win, a->win_host))
    return e;
  SceneD d;
  d.src = a->src; d.win = a->win; d.out = a->out;
  d.cs = a->chan_stride; d.rs = a->row_stride; d.xs = a->col_stride;
  d.C = a->C; d.H = a->H; d.W = a->W; d.pad_top = a->pad_top; d.pad_left = a->pad_left;
  d.vpr = (unsigned)(a->win_w / 4);
  d.vpp = d.vpr * (unsigned)a->win_h;
  d.chunks = (d.vpp + SG_CHUNK - 1) / SG_CHUNK;
  d.scale = a->scale;
  const long long blocks = (long long)a->n * a->C * d.chunks;
  SC_REQUIRE(blocks <= INT_MAX, "sc_scene_gather: grid of %lld work-groups is too large for one launch", blocks);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), wg(SG_WG);
  const bool sc = a->scale != 1.0f;
  if (a->elem_bytes == 2) {
    if (sc) hipLaunchKernelGGL((k_scene_gather<uint16_t, true>), grid, wg, 0, st, d);
    else hipLaunchKernelGGL((k_scene_gather<uint16_t, false>), grid, wg, 0, st, d);
  } else {
    if (sc) hipLaunchKernelGGL((k_scene_gather<float, true>), grid, wg, 0, st, d);
    else hipLaunchKernelGGL((k_scene_gather<float, false>), grid, wg, 0, st, d);
  }
  SC_LAUNCH_OK("sc_scene_gather");
  return SC_OK;
}
