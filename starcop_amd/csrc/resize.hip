// Anti-aliased downscaling of simulated sensor bands to the sensor's pixel size: what georeader's read.resize(..., anti_aliasing=True,
// anti_aliasing_sigma=sigma_bands) leaves at the end of starcop/data/aviris.py:262-338 (transform_to_srf), i.e. per plane
//   scipy.ndimage.zoom(scipy.ndimage.gaussian_filter(x, (sy, sx), mode, cval), (oh / H, ow / W), order=1, mode, cval, grid_mode=True).
// The operator is separable and linear in (x, cval): per axis, output j = sum_k w[j][k] * x[start[j] + k] + wc[j] * cval with at most
// min(n, 2 radius + 2) contiguous in-range taps (the two shifted Gaussians of the bilinear lerp, folded back into the axis by the border
// rule); the tables are built on the host in float64 (starcop_amd/resample.py: axis_taps).  Two launches for all planes of a call:
//   vertical   : a work-group owns a strip of 64 columns and a run of output lines; the input lines of the run are staged ONCE into LDS
//                with lines coalesced along samples (16-byte loads where the layout allows), then wave v computes output lines v, v + 4,
//                .. with one lane per column -- the tap weights are wave-uniform (held one per lane and broadcast, see tap_sum), the LDS reads
//                conflict-free.  Writes the float32 intermediate [P][oh][W].
//   horizontal : a work-group owns 64 lines x a run of output columns of the intermediate (H / oh times smaller than the input); the
//                source columns of the run are staged into LDS with an odd pitch, one lane per LINE, so the weights are wave-uniform here
//                too and lanes hit distinct banks; the results cross LDS once more so that the stores are contiguous along samples.
// Arithmetic (the contract of srf.hip): each product in fp64 with the float32 value promoted exactly, added in ascending tap order onto a
// +0.0 seed, wc * cval added last, never an FMA, rounded once to float32 at the end of each pass: bit-equal to a numpy loop over the taps,
// identical between calls and between a plane alone and inside a batch.  No atomics.
#include <limits.h>

#include "sc_common.h"

namespace {

constexpr int RS_WG = 256;                 // four waves
constexpr int RS_CW = 64;                  // columns of a vertical strip / lines of a horizontal tile: one per lane
constexpr int RS_T_MAX = 256;
constexpr int RS_LDS_SOFT = 64 * 1024;     // the runs shrink until their staging fits this; a single output may still need more
constexpr int RS_LDS_MAX = 160 * 1024;
constexpr int RS_STAGE = 8;                // loads in flight per thread while staging
constexpr int RS_STAGE_V = 8;              // .. 16-byte loads of the vertical pass: a run of 16 lines at ratio 4 and 46 taps in one round trip
// output lines per work-group of the vertical pass, at most.  16 against 32 on the 13-band 5 m -> 20 m flight line: 0.360 against 0.403 ms
// per call -- 27 KB of staging instead of 44 KB puts five work-groups on a CU instead of three, and the staging of one then runs under
// the fp64 taps of the others; that outweighs the lines read twice at the seams of the shorter runs (106 staged for 64 new at 46 taps)
constexpr int RS_RUN_V = 16;
constexpr int RS_RUN_H = 16;               // output columns per work-group of the horizontal pass, at most
constexpr int RS_RPW_V = RS_RUN_V / (RS_WG / 64);   // outputs per wave
constexpr int RS_RPW_H = RS_RUN_H / (RS_WG / 64);

struct AxisD {
  int n, o, T, n_tables;
  const int32_t* start;
  const int32_t* taps;       // may be NULL: T
  const double* w;
  const double* wc;
  const int32_t* table;      // [P]
};

struct ResD {
  const float* x;
  long long xps, xls, xss;   // element strides of plane, line, sample
  float* tmp;                // [P][oh][W]
  float* out;
  long long ops, ols;
  int H, W, oh, ow;
  float cval;
  AxisD y, xa;
  int run;                   // outputs of the axis per work-group
  int rows;                  // vertical: LDS lines; horizontal: LDS pitch (odd)
};

// sum_k w[k] * get(k) + wc * cval.  hipcc contracts a * b + c into v_fma_f64 by default (-ffp-contract=fast): scoped off here, as in
// srf_pixel.
// The weights of an output are wave-uniform.  Read as scalar loads inside the tap loop they share the wait counter of the LDS reads, and
// a scalar load can only be waited for by draining that counter, so every few taps the wave sat out a scalar-cache round trip.  Instead
// lane k holds w[k] (one coalesced load per output, issued before the staging barrier) and tap k broadcasts it with v_readlane; rows of
// more than 64 taps (sigma above 7.75) reload in the loop.  All lanes of the wave must be active here.
__device__ __forceinline__ double lane_weights(const double* __restrict__ w, int k0, int nt, int lane) {
  return k0 + lane < nt ? w[k0 + lane] : 0.0;
}
__device__ __forceinline__ double lane_bcast(double v, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}
template <class Get>
__device__ __forceinline__ float tap_sum(const double* __restrict__ w, double w0, int lane, int nt, double wc, double cval, Get get) {
#pragma clang fp contract(off)
  double acc = 0.0;
  double wv = w0;
  for (int k0 = 0; k0 < nt; k0 += 64) {
    if (k0) wv = lane_weights(w, k0, nt, lane);
    const int n = min(64, nt - k0);
    // unrolled by hand: the broadcast is a convergent operation, which keeps the compiler from unrolling a loop of unknown length
#define RS_TAP(kk)                                                    \
  {                                                                   \
    const double p = lane_bcast(wv, (kk)) * (double)get(k0 + (kk));   \
    acc = acc + p;                                                    \
  }
    int k = 0;
    for (; k + 4 <= n; k += 4) {
      RS_TAP(k) RS_TAP(k + 1) RS_TAP(k + 2) RS_TAP(k + 3)
    }
    for (; k < n; ++k) RS_TAP(k)
#undef RS_TAP
  }
  const double c = wc * cval;
  acc = acc + c;
  return __double2float_rn(acc);
}

// table, tap count and source window [lo, lo + cnt) of the outputs [j0, j1) of one plane.  The host has checked its copy of the tables;
// the clamps keep a device copy that differs from touching memory outside the plane or the staging buffer.
struct Window { int tab, nt, lo, cnt; };
__device__ __forceinline__ Window axis_window(const AxisD& ax, int plane, int j0, int j1, int cap) {
  Window v;
  v.tab = min(max(ax.table[plane], 0), ax.n_tables - 1);
  const int tmax = min(min(ax.T, ax.n), cap);
  v.nt = ax.taps ? min(max(ax.taps[v.tab], 1), tmax) : tmax;
  const int32_t* st = ax.start + (size_t)v.tab * ax.o;
  int lo = INT_MAX, hi = 0;
  for (int j = j0; j < j1; ++j) {
    const int s = st[j];
    lo = min(lo, s);
    hi = max(hi, s + v.nt);
  }
  v.lo = min(max(lo, 0), ax.n - v.nt);
  v.cnt = min(min(max(hi - v.lo, v.nt), cap), ax.n - v.lo);
  return v;
}

// grid.x = chunks of a.run output lines x strips of 64 columns (strips fastest), grid.y = plane; LDS [a.rows][64] floats
template <bool VEC>
__global__ __launch_bounds__(RS_WG) void k_resize_v(ResD a, int strips) {
  extern __shared__ __attribute__((aligned(16))) float win[];
  const int chunk = blockIdx.x / strips;
  const int c0 = (blockIdx.x - chunk * strips) * RS_CW;
  const int p = blockIdx.y;
  const int j0 = chunk * a.run, j1 = min(j0 + a.run, a.oh);
  const Window v = axis_window(a.y, p, j0, j1, a.rows);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // this wave's outputs j0 + wave + 4 i: window offset, cval weight and the lane's tap weight, in flight while the lines are staged
  const size_t trow = (size_t)v.tab * a.oh;
  int so[RS_RPW_V];
  double wco[RS_RPW_V], w0[RS_RPW_V];
#pragma unroll
  for (int i = 0; i < RS_RPW_V; ++i) {
    const int j = min(j0 + wave + i * (RS_WG / 64), a.oh - 1);
    so[i] = min(max(a.y.start[trow + j] - v.lo, 0), v.cnt - v.nt);
    wco[i] = a.y.wc[trow + j];
    w0[i] = lane_weights(a.y.w + (trow + j) * a.y.T, 0, v.nt, lane);
  }
  const float* src = a.x + (long long)p * a.xps + (long long)v.lo * a.xls;
  if (VEC) {
    // sample stride 1, every line start 16-byte aligned, W a multiple of 4: thread t takes granule t & 15 of line t >> 4
    const int total = v.cnt * (RS_CW / 4);
    for (int q0 = threadIdx.x; q0 < total; q0 += RS_WG * RS_STAGE_V) {
      float4 r[RS_STAGE_V];
#pragma unroll
      for (int u = 0; u < RS_STAGE_V; ++u) {
        const int q = q0 + u * RS_WG;
        const int col = c0 + (q & 15) * 4;
        r[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < total && col < a.W) r[u] = *reinterpret_cast<const float4*>(src + (long long)(q >> 4) * a.xls + col);
      }
#pragma unroll
      for (int u = 0; u < RS_STAGE_V; ++u) {
        const int q = q0 + u * RS_WG;
        if (q < total) *reinterpret_cast<float4*>(win + (size_t)q * 4) = r[u];
      }
    }
  } else {
    const int total = v.cnt * RS_CW;
    for (int q0 = threadIdx.x; q0 < total; q0 += RS_WG * RS_STAGE) {
      float r[RS_STAGE];
#pragma unroll
      for (int u = 0; u < RS_STAGE; ++u) {
        const int q = q0 + u * RS_WG;
        const int col = c0 + (q & 63);
        r[u] = 0.f;
        if (q < total && col < a.W) r[u] = src[(long long)(q >> 6) * a.xls + (long long)col * a.xss];
      }
#pragma unroll
      for (int u = 0; u < RS_STAGE; ++u) {
        const int q = q0 + u * RS_WG;
        if (q < total) win[q] = r[u];
      }
    }
  }
  __syncthreads();
  const bool live = c0 + lane < a.W;
  const double cv = (double)a.cval;
#pragma unroll
  for (int i = 0; i < RS_RPW_V; ++i) {
    const int j = j0 + wave + i * (RS_WG / 64);
    if (j >= j1) break;                                  // wave-uniform
    const float* col = win + so[i] * RS_CW + lane;
    const float r = tap_sum(a.y.w + (trow + j) * a.y.T, w0[i], lane, v.nt, wco[i], cv, [&](int k) { return col[k * RS_CW]; });
    if (live) a.tmp[((size_t)p * a.oh + j) * a.W + c0 + lane] = r;
  }
}

// grid.x = tiles of 64 lines x chunks of a.run output columns (chunks fastest), grid.y = plane; LDS [64][pitch] source floats (pitch =
// a.rows, odd) followed by [64][a.run + 1] results
__global__ __launch_bounds__(RS_WG) void k_resize_h(ResD a, int chunks) {
  extern __shared__ __attribute__((aligned(16))) float win[];
  const int tile = blockIdx.x / chunks;
  const int i0 = (blockIdx.x - tile * chunks) * a.run, i1 = min(i0 + a.run, a.ow);
  const int p = blockIdx.y;
  const int r0 = tile * RS_CW, nr = min(RS_CW, a.oh - r0);
  const int pitch = a.rows;
  const Window v = axis_window(a.xa, p, i0, i1, pitch);
  float* res = win + RS_CW * pitch;
  const int opitch = a.run + 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t trow = (size_t)v.tab * a.ow;
  int so[RS_RPW_H];
  double wco[RS_RPW_H], w0[RS_RPW_H];
#pragma unroll
  for (int u = 0; u < RS_RPW_H; ++u) {
    const int i = min(i0 + wave + u * (RS_WG / 64), a.ow - 1);
    so[u] = min(max(a.xa.start[trow + i] - v.lo, 0), v.cnt - v.nt);
    wco[u] = a.xa.wc[trow + i];
    w0[u] = lane_weights(a.xa.w + (trow + i) * a.xa.T, 0, v.nt, lane);
  }
  const float* src = a.tmp + ((size_t)p * a.oh + r0) * a.W + v.lo;
  // wave w stages lines w, w + 4, ..: RS_STAGE of them in flight per thread before any goes to LDS
  for (int cb = 0; cb < v.cnt; cb += 64) {
    const int c = cb + lane;
    for (int rb = wave; rb < nr; rb += (RS_WG / 64) * RS_STAGE) {
      float t[RS_STAGE];
#pragma unroll
      for (int u = 0; u < RS_STAGE; ++u) {
        const int r = rb + u * (RS_WG / 64);
        t[u] = 0.f;
        if (r < nr && c < v.cnt) t[u] = src[(size_t)r * a.W + c];
      }
#pragma unroll
      for (int u = 0; u < RS_STAGE; ++u) {
        const int r = rb + u * (RS_WG / 64);
        if (r < nr && c < v.cnt) win[r * pitch + c] = t[u];
      }
    }
  }
  __syncthreads();
  // every lane computes (lanes past the last line read staging rows nobody filled and their results are never stored): the weight
  // broadcast needs the whole wave
  const double cv = (double)a.cval;
#pragma unroll
  for (int u = 0; u < RS_RPW_H; ++u) {
    const int i = i0 + wave + u * (RS_WG / 64);
    if (i >= i1) break;                                  // wave-uniform
    const float* row = win + lane * pitch + so[u];
    res[lane * opitch + i - i0] = tap_sum(a.xa.w + (trow + i) * a.xa.T, w0[u], lane, v.nt, wco[u], cv, [&](int k) { return row[k]; });
  }
  __syncthreads();
  const int nc = i1 - i0;
  float* dst = a.out + (long long)p * a.ops + (long long)r0 * a.ols + i0;
  for (int q = threadIdx.x; q < nr * a.run; q += RS_WG) {
    const int r = q / a.run, c = q - r * a.run;
    if (c < nc) dst[(long long)r * a.ols + c] = res[r * opitch + c];
  }
}

// host: the widest source window any run of `run` outputs of any table needs
int widest_window(const sc_resize_axis& ax, int run) {
  int widest = 0;
  for (int t = 0; t < ax.n_tables; ++t) {
    const int nt = ax.taps_host ? ax.taps_host[t] : ax.T;
    const int32_t* st = ax.start_host + (size_t)t * ax.o;
    for (int j0 = 0; j0 < ax.o; j0 += run) {
      int lo = INT_MAX, hi = 0;
      for (int j = j0; j < min(j0 + run, ax.o); ++j) {
        lo = min(lo, st[j]);
        hi = max(hi, st[j] + nt);
      }
      widest = max(widest, hi - lo);
    }
  }
  return widest;
}

int check_axis(const sc_resize_axis& ax, const int32_t* table_host, int P, const char* name) {
  SC_REQUIRE(ax.n >= 1 && ax.o >= 1, "sc_resize_aa: %s axis: bad lengths n=%d o=%d", name, ax.n, ax.o);
  SC_REQUIRE(ax.o <= ax.n, "sc_resize_aa: %s axis: output %d larger than input %d (downscaling only)", name, ax.o, ax.n);
  SC_REQUIRE(ax.T >= 1 && ax.T <= RS_T_MAX, "sc_resize_aa: %s axis: T=%d outside [1, %d]", name, ax.T, RS_T_MAX);
  SC_REQUIRE(ax.n_tables >= 1 && ax.n_tables <= 65535, "sc_resize_aa: %s axis: n_tables=%d outside [1, 65535]", name, ax.n_tables);
  SC_REQUIRE(ax.start && ax.w && ax.wc && ax.start_host && (!ax.taps == !ax.taps_host), "sc_resize_aa: %s axis: null table pointer", name);
  for (int t = 0; t < ax.n_tables; ++t) {
    const int nt = ax.taps_host ? ax.taps_host[t] : ax.T;
    SC_REQUIRE(nt >= 1 && nt <= ax.T, "sc_resize_aa: %s axis: table %d uses %d taps, outside [1, T=%d]", name, t, nt, ax.T);
    const int32_t* st = ax.start_host + (size_t)t * ax.o;
    for (int j = 0; j < ax.o; ++j)
      SC_REQUIRE(st[j] >= 0 && st[j] <= ax.n - nt, "sc_resize_aa: %s axis: taps [%d, %d) of output %d (table %d) leave [0, %d)", name,
                 st[j], st[j] + nt, j, t, ax.n);
  }
  for (int p = 0; p < P; ++p)
    SC_REQUIRE(table_host[p] >= 0 && table_host[p] < ax.n_tables, "sc_resize_aa: %s axis: plane %d uses table %d of %d", name, p,
               table_host[p], ax.n_tables);
  return SC_OK;
}

AxisD to_axisd(const sc_resize_axis& ax, const int32_t* table) {
  AxisD d;
  d.n = ax.n; d.o = ax.o; d.T = ax.T; d.n_tables = ax.n_tables;
  d.start = ax.start; d.taps = ax.taps; d.w = ax.w; d.wc = ax.wc; d.table = table;
  return d;
}

}  // namespace

extern "C" size_t sc_resize_workspace_bytes(int P, int oh, int W) {
  if (P < 1 || oh < 1 || W < 1) return 0;
  return (size_t)P * (size_t)oh * (size_t)W * sizeof(float);
}

extern "C" int sc_resize_aa(const sc_resize_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_resize_aa: null arguments");
  SC_REQUIRE(a->x && a->out && a->work && a->table_y && a->table_x && a->table_y_host && a->table_x_host, "sc_resize_aa: null pointer");
  SC_REQUIRE(a->P >= 1 && a->P <= 65535, "sc_resize_aa: P=%d outside [1, 65535]", a->P);
  SC_REQUIRE(a->plane_stride >= 0 && a->line_stride >= 0 && a->sample_stride >= 0 && a->out_plane_stride >= 0 &&
                 a->out_line_stride >= 0, "sc_resize_aa: negative stride");
  int rc = check_axis(a->y, a->table_y_host, a->P, "line");
  if (rc) return rc;
  rc = check_axis(a->xs, a->table_x_host, a->P, "sample");
  if (rc) return rc;
  const int H = a->y.n, oh = a->y.o, W = a->xs.n, ow = a->xs.o;
  SC_REQUIRE(a->work_bytes >= sc_resize_workspace_bytes(a->P, oh, W), "sc_resize_aa: workspace of %zu bytes, %zu needed", a->work_bytes,
             sc_resize_workspace_bytes(a->P, oh, W));
  SC_REQUIRE((uintptr_t)a->work % 4 == 0 && (uintptr_t)a->x % 4 == 0 && (uintptr_t)a->out % 4 == 0, "sc_resize_aa: misaligned pointer");

  ResD d;
  d.x = a->x; d.xps = a->plane_stride; d.xls = a->line_stride; d.xss = a->sample_stride;
  d.tmp = (float*)a->work; d.out = a->out; d.ops = a->out_plane_stride; d.ols = a->out_line_stride;
  d.H = H; d.W = W; d.oh = oh; d.ow = ow; d.cval = a->cval;
  d.y = to_axisd(a->y, a->table_y);
  d.xa = to_axisd(a->xs, a->table_x);
  hipStream_t st = (hipStream_t)stream;

  // vertical: runs of up to RS_RUN_V output lines, halved until the staged lines fit the soft LDS budget (one output needs at most T lines)
  int run = RS_RUN_V, rows = widest_window(a->y, run);
  while (run > 1 && (size_t)rows * RS_CW * sizeof(float) > (size_t)RS_LDS_SOFT) {
    run >>= 1;
    rows = widest_window(a->y, run);
  }
  size_t lds = (size_t)rows * RS_CW * sizeof(float);
  SC_REQUIRE(lds <= (size_t)RS_LDS_MAX, "sc_resize_aa: line window of %d lines does not fit the LDS", rows);
  const int strips = (W + RS_CW - 1) / RS_CW;
  long long blocks = (long long)strips * ((oh + run - 1) / run);
  SC_REQUIRE(blocks <= INT_MAX, "sc_resize_aa: planes too large for one launch");
  d.run = run; d.rows = rows;
  const bool vec = a->sample_stride == 1 && W % 4 == 0 && a->line_stride % 4 == 0 && a->plane_stride % 4 == 0 && (uintptr_t)a->x % 16 == 0;
  if (vec) {
    SC_REQUIRE(sc_lds_limit(&k_resize_v<true>, lds, "sc_resize_aa") == SC_OK, "sc_resize_aa: cannot raise the LDS limit of the vertical pass");
    hipLaunchKernelGGL(k_resize_v<true>, dim3((unsigned)blocks, (unsigned)a->P), dim3(RS_WG), lds, st, d, strips);
  } else {
    SC_REQUIRE(sc_lds_limit(&k_resize_v<false>, lds, "sc_resize_aa") == SC_OK, "sc_resize_aa: cannot raise the LDS limit of the vertical pass");
    hipLaunchKernelGGL(k_resize_v<false>, dim3((unsigned)blocks, (unsigned)a->P), dim3(RS_WG), lds, st, d, strips);
  }
  SC_LAUNCH_OK("sc_resize_aa (vertical)");

  // horizontal: runs of up to RS_RUN_H output columns, 64 lines per work-group
  run = RS_RUN_H;
  int pitch = widest_window(a->xs, run) | 1;
  while (run > 1 && ((size_t)pitch + run + 1) * RS_CW * sizeof(float) > (size_t)RS_LDS_SOFT) {
    run >>= 1;
    pitch = widest_window(a->xs, run) | 1;
  }
  lds = ((size_t)pitch + run + 1) * RS_CW * sizeof(float);
  SC_REQUIRE(lds <= (size_t)RS_LDS_MAX, "sc_resize_aa: sample window of %d samples does not fit the LDS", pitch);
  const int chunks = (ow + run - 1) / run;
  blocks = (long long)chunks * ((oh + RS_CW - 1) / RS_CW);
  SC_REQUIRE(blocks <= INT_MAX, "sc_resize_aa: planes too large for one launch");
  d.run = run; d.rows = pitch;
  SC_REQUIRE(sc_lds_limit(&k_resize_h, lds, "sc_resize_aa") == SC_OK, "sc_resize_aa: cannot raise the LDS limit of the horizontal pass");
  hipLaunchKernelGGL(k_resize_h, dim3((unsigned)blocks, (unsigned)a->P), dim3(RS_WG), lds, st, d, chunks);
  SC_LAUNCH_OK("sc_resize_aa (horizontal)");
  return SC_OK;
}
