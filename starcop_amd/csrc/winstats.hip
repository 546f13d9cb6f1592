// Window statistics of a mag1c flight line (scripts/preprocessing/stats_mag1c.py:41-63): for every window of a scene the ten
// statistics max, min, mean, percentile 1 / 5 / 50 / 95 / 99, sum, count of the value set
//   V = { min(v, clip_max) : v in window, v != fill, v >= 0 }
// The windows are strided views of ONE scene (every pixel lies in up to four of them) and each has its own count, hence its own
// ranks: the ten order statistics a window needs (two neighbours for each of the four percentiles, two middles for the median)
// are found together by an exact radix select on the float bit patterns.  Members of V are non-negative, so their bit patterns
// are ordered as integers and fit 31 bits: three passes of 11 + 10 + 10 bits (the first digit is the exponent and the top three
// mantissa bits -- at clip_max = 10 000 only 1 122 of its 2 048 bins can be hit) instead of four passes of 8.
//   k_ws_pass<0>  count / min / max / fp64 sum of a chunk of rows of a window, histogram of digit 0
//   k_ws_pick<0>  reduces the chunks in a fixed order, derives the ten ranks from the count, picks digit 0 of every rank
//   k_ws_pass<1>, k_ws_pick<1>, k_ws_pass<2>, k_ws_pick<2>: digits 1 and 2, every distinct prefix of the ten ranks has a histogram
//                 of its own (neighbouring ranks nearly always share one); the last pick interpolates and writes the outputs.
// A pass is grid = n_win x nchunk work-groups, each reading its rows of the scene in place (the scene stays in the last-level
// cache across windows and passes); histograms are LDS integer atomics flushed to global integer atomics -- exact and order-
// independent.  The sums use no atomics: per-lane serial fp64 in a fixed pixel order, one butterfly, the waves and then the chunks
// added in index order, so repeated calls give identical bits.
// Interpolation: what numpy >= 2.0 computes for float32 data -- the quantile, the virtual index, the weight and the two-sided lerp
// are all float32 (np_lerp below); the median is the float32 mean of the two middle order statistics.
#include <limits.h>
#include <math.h>

#include "sc_common.h"

// numpy rounds every float32 operation of the virtual index, the weight and the lerp: nothing here may become an FMA
#pragma clang fp contract(off)

namespace {

constexpr int WS_R = 10;                // order statistics per window
constexpr int WS_WG = 256;
constexpr int WS_BINS0 = 2048;          // digit 0: key >> 20
constexpr int WS_BINS = 1024;           // digits 1 and 2: 10 bits each
constexpr int WS_MAX_CHUNKS = 64;

struct WsState {                        // per window, lives in the workspace between launches
  unsigned k[WS_R];                     // rank of each order statistic among the keys that share its prefix
  unsigned prefix[WS_R];                // resolved high bits of each order statistic (right-aligned)
  unsigned slot_prefix[WS_R];           // the distinct prefixes ...
  int rank_slot[WS_R];                  // ... and which of them each rank uses
  int nslot;                            // 0: empty window, nothing to select
  int pad;
  long long count;
};
struct WsPart { double sum; long long count; float mn, mx; };

struct WsD {
  const float* x;
  long long rs;                         // row stride, elements
  int H, W, n_win, nchunk;
  const int32_t* win;                   // [n_win][4] row_off, col_off, height, width
  int has_fill;
  float fill, clip;
  WsState* st;
  WsPart* part;                         // [n_win][nchunk]
  unsigned* hist0;                      // [n_win][WS_BINS0]
  unsigned* hist;                       // [n_win][WS_R][WS_BINS]
  int64_t* count;
  double* sum_mean;                     // [n_win][2]
  float* stats;                         // [n_win][7] max, min, p01, p05, p50, p95, p99
  float q32[4];                         // float32(q) / float32(100) for q = 1, 5, 95, 99
};

// rows [r0, r1) x cols [c0, c0 + w) of this work-group; the device copy of the window is clamped to the scene, so a list that
// differs from the host copy the entry point checked still cannot read outside it
__device__ __forceinline__ void ws_rows(const WsD& a, int wi, int chunk, int& r0, int& r1, int& c0, int& w) {
  const int32_t* q = a.win + (size_t)wi * 4;
  const int ro = min(max(q[0], 0), a.H), co = min(max(q[1], 0), a.W);
  const int h = min(max(q[2], 0), a.H - ro);
  w = min(max(q[3], 0), a.W - co);
  c0 = co;
  const int rpc = (h + a.nchunk - 1) / a.nchunk;
  r0 = ro + min(chunk * rpc, h);
  r1 = ro + min(chunk * rpc + rpc, h);
}

// member of V -> key (true), anything else -> false.  -0.0 passes v >= 0 as in numpy and sorts with +0.0: its key is 0.
__device__ __forceinline__ bool ws_key(const WsD& a, float v, float& c, unsigned& key) {
  const bool ok = (!a.has_fill || v != a.fill) && v >= 0.f;
  c = fminf(v, a.clip);
  key = __float_as_uint(c) & 0x7FFFFFFFu;
  return ok;
}

template <int PASS>
__global__ __launch_bounds__(WS_WG) void k_ws_pass(WsD a) {
  __shared__ unsigned h[PASS == 0 ? WS_BINS0 : WS_R * WS_BINS];
  __shared__ WsPart s_part[WS_WG / 64];
  const int wi = blockIdx.x / a.nchunk, chunk = blockIdx.x - wi * a.nchunk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const WsState* st = a.st + wi;
  const int nslot = PASS == 0 ? 1 : st->nslot;
  if (PASS != 0 && nslot == 0) return;
  const int nb = PASS == 0 ? WS_BINS0 : nslot * WS_BINS;
  for (int i = threadIdx.x; i < nb; i += WS_WG) h[i] = 0;
  __syncthreads();
  int r0, r1, c0, w;
  ws_rows(a, wi, chunk, r0, r1, c0, w);
  unsigned sp[WS_R];
  if (PASS != 0) {
#pragma unroll
    for (int s = 0; s < WS_R; ++s) sp[s] = st->slot_prefix[s];
  }
  double sum = 0.0;
  long long cnt = 0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int r = r0 + wave; r < r1; r += WS_WG / 64) {
    const float* row = a.x + (long long)r * a.rs + c0;
    for (int c = lane; c < w; c += 64 * 4) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = c + 64 * u < w ? row[c + 64 * u] : -1.f;      // -1: not a member of V
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float cv;
        unsigned key;
        if (!ws_key(a, v[u], cv, key)) continue;
        if (PASS == 0) {
          sum += (double)cv; ++cnt; mn = fminf(mn, cv); mx = fmaxf(mx, cv);
          atomicAdd(&h[key >> 20], 1u);
        } else {
          const unsigned pre = PASS == 1 ? key >> 20 : key >> 10;
          const unsigned dig = PASS == 1 ? (key >> 10) & 1023u : key & 1023u;
          for (int s = 0; s < nslot; ++s)
            if (pre == sp[s]) { atomicAdd(&h[s * WS_BINS + dig], 1u); break; }
        }
      }
    }
  }
  if (PASS == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o, 64);
      cnt += __shfl_xor(cnt, o, 64);
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) { s_part[wave].sum = sum; s_part[wave].count = cnt; s_part[wave].mn = mn; s_part[wave].mx = mx; }
  }
  __syncthreads();
  if (PASS == 0 && threadIdx.x == 0) {
    WsPart p = s_part[0];
    for (int v = 1; v < WS_WG / 64; ++v) {
      p.sum += s_part[v].sum; p.count += s_part[v].count; p.mn = fminf(p.mn, s_part[v].mn); p.mx = fmaxf(p.mx, s_part[v].mx);
    }
    a.part[(size_t)wi * a.nchunk + chunk] = p;
  }
  unsigned* g = PASS == 0 ? a.hist0 + (size_t)wi * WS_BINS0 : a.hist + (size_t)wi * WS_R * WS_BINS;
  for (int i = threadIdx.x; i < nb; i += WS_WG) {
    const unsigned v = h[i];
    if (v) atomicAdd(g + i, v);
  }
}

// numpy's _lerp on float32 operands: every operation rounds to float32, none is fused
__device__ __forceinline__ float np_lerp(float a, float b, float t) {
  const float d = b - a;
  float r = a + d * t;
  if (t >= 0.5f) r = b - d * (1.0f - t);
  return r;
}

// One work-group per window.  For every histogram in use: an exclusive scan over its bins (each thread owns NB / 256 consecutive
// bins; Hillis-Steele over the thread totals in LDS), then the thread whose bins hold rank k of an order statistic records the
// digit.  Clears what it read, so the next pass finds zeros.
template <int PASS>
__global__ __launch_bounds__(WS_WG) void k_ws_pick(WsD a) {
  constexpr int NB = PASS == 0 ? WS_BINS0 : WS_BINS;
  constexpr int PER = NB / WS_WG;
  __shared__ unsigned scan[2][WS_WG];
  __shared__ unsigned new_prefix[WS_R], new_k[WS_R];
  __shared__ WsState s;
  const int wi = blockIdx.x, t = threadIdx.x;
  WsState* st = a.st + wi;
  if (t == 0) {
    if (PASS == 0) {
      const WsPart* p = a.part + (size_t)wi * a.nchunk;
      double sum = 0.0;
      long long cnt = 0;
      float mn = __builtin_inff(), mx = -__builtin_inff();
      for (int c = 0; c < a.nchunk; ++c) { sum += p[c].sum; cnt += p[c].count; mn = fminf(mn, p[c].mn); mx = fmaxf(mx, p[c].mx); }
      a.count[wi] = cnt;
      for (int r = 0; r < WS_R; ++r) { s.k[r] = 0; s.prefix[r] = 0; s.rank_slot[r] = 0; s.slot_prefix[r] = 0; }
      s.count = cnt;
      s.pad = 0;
      s.nslot = cnt > 0 ? 1 : 0;
      if (cnt == 0) {
        a.sum_mean[(size_t)wi * 2] = a.sum_mean[(size_t)wi * 2 + 1] = __builtin_nan("");
        for (int j = 0; j < 7; ++j) a.stats[(size_t)wi * 7 + j] = __builtin_nanf("");
      } else {
        a.sum_mean[(size_t)wi * 2] = sum;
        a.sum_mean[(size_t)wi * 2 + 1] = sum / (double)cnt;
        a.stats[(size_t)wi * 7] = mx;
        a.stats[(size_t)wi * 7 + 1] = mn;
        // ranks: percentiles 1, 5 -> 0..3, median -> 4, 5, percentiles 95, 99 -> 6..9
        const unsigned last = (unsigned)(cnt - 1);
        for (int j = 0; j < 4; ++j) {
          const float vi = (float)(cnt - 1) * a.q32[j];
          const unsigned lo = min((unsigned)floorf(vi), last);
          const int r = j < 2 ? 2 * j : 2 * j + 2;
          s.k[r] = lo;
          s.k[r + 1] = min(lo + 1u, last);
        }
        s.k[4] = (cnt & 1) ? (unsigned)((cnt - 1) / 2) : (unsigned)(cnt / 2 - 1);
        s.k[5] = (unsigned)(cnt / 2);
      }
    } else {
      s = *st;
    }
  }
  if (t < WS_R) { new_prefix[t] = 0; new_k[t] = 0; }
  __syncthreads();
  const int nslot = s.nslot;
  for (int sl = 0; sl < nslot; ++sl) {
    unsigned* g = (PASS == 0 ? a.hist0 + (size_t)wi * WS_BINS0 : a.hist + ((size_t)wi * WS_R + sl) * WS_BINS) + t * PER;
    unsigned c[PER], tot = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) { c[i] = g[i]; g[i] = 0; tot += c[i]; }
    int cur = 0;
    scan[0][t] = tot;
    __syncthreads();
    for (int o = 1; o < WS_WG; o <<= 1) {
      scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0u);
      cur ^= 1;
      __syncthreads();
    }
    const unsigned before = scan[cur][t] - tot;              // keys in the bins of lower threads
    for (int r = 0; r < WS_R; ++r) {
      if (s.rank_slot[r] != sl) continue;
      const unsigned k = s.k[r];
      if (k < before || k >= before + tot) continue;
      unsigned cum = before;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        if (k >= cum && k < cum + c[i]) {
          new_prefix[r] = (s.prefix[r] << (PASS == 0 ? 11 : 10)) | (unsigned)(t * PER + i);
          new_k[r] = k - cum;
        }
        cum += c[i];
      }
    }
    __syncthreads();
  }
  if (t != 0) return;
  if (nslot == 0) {
    if (PASS == 0) *st = s;
    return;
  }
  if (PASS < 2) {
    // the distinct prefixes of the ten ranks: one histogram each in the next pass
    int n = 0;
    for (int r = 0; r < WS_R; ++r) {
      s.prefix[r] = new_prefix[r];
      s.k[r] = new_k[r];
      int sl = -1;
      for (int q = 0; q < n; ++q)
        if (s.slot_prefix[q] == new_prefix[r]) sl = q;
      if (sl < 0) { sl = n; s.slot_prefix[n++] = new_prefix[r]; }
      s.rank_slot[r] = sl;
    }
    s.nslot = n;
    *st = s;
  } else {
    float v[WS_R];
    for (int r = 0; r < WS_R; ++r) v[r] = __uint_as_float(new_prefix[r]);
    float* o = a.stats + (size_t)wi * 7;
    for (int j = 0; j < 4; ++j) {
      const float vi = (float)(s.count - 1) * a.q32[j];
      const float g = s.count > 1 ? vi - floorf(vi) : 0.f;
      const int r = j < 2 ? 2 * j : 2 * j + 2;
      o[j < 2 ? 2 + j : 3 + j] = np_lerp(v[r], v[r + 1], g);
    }
    o[4] = (v[4] + v[5]) / 2.0f;
  }
}

size_t ws_align(size_t v) { return (v + 255) & ~(size_t)255; }
int ws_chunks(int n_win) {
  const int c = (2048 + n_win - 1) / n_win;
  return c < 1 ? 1 : (c > WS_MAX_CHUNKS ? WS_MAX_CHUNKS : c);
}

}  // namespace

extern "C" size_t sc_window_stats_workspace_bytes(int n_win) {
  if (n_win <= 0) return 0;
  const size_t n = (size_t)n_win;
  return ws_align(n * sizeof(WsState)) + ws_align(n * ws_chunks(n_win) * sizeof(WsPart)) + ws_align(n * WS_BINS0 * sizeof(unsigned)) +
         ws_align(n * WS_R * WS_BINS * sizeof(unsigned));
}

extern "C" int sc_window_stats(const sc_winstats_args* a, void* work, size_t work_bytes, sc_stream stream) {
  SC_REQUIRE(a, "sc_window_stats: null arguments");
  SC_REQUIRE(a->x && a->windows && a->windows_host && a->count && a->sum_mean && a->stats && work, "sc_window_stats: null pointer");
  SC_REQUIRE(a->H >= 1 && a->W >= 1 && (long long)a->H * a->W < (1ll << 31), "sc_window_stats: bad scene dims H=%d W=%d", a->H, a->W);
  SC_REQUIRE(a->row_stride >= a->W, "sc_window_stats: row stride %lld smaller than the width %d", (long long)a->row_stride, a->W);
  SC_REQUIRE(a->n_win >= 1 && a->n_win <= (1 << 20), "sc_window_stats: n_win=%d outside [1, 2^20]", a->n_win);
  SC_REQUIRE(a->clip_max >= 0.f, "sc_window_stats: clip_max must be >= 0 (and not NaN)");
  for (int i = 0; i < a->n_win; ++i) {
    const int32_t* q = a->windows_host + (size_t)i * 4;
    SC_REQUIRE(q[2] >= 1 && q[3] >= 1, "sc_window_stats: window %d has height %d, width %d", i, q[2], q[3]);
    SC_REQUIRE(q[0] >= 0 && q[1] >= 0 && (long long)q[0] + q[2] <= a->H && (long long)q[1] + q[3] <= a->W,
               "sc_window_stats: window %d (row %d, col %d, %d x %d) is not inside the %d x %d scene", i, q[0], q[1], q[2], q[3], a->H, a->W);
  }
  SC_REQUIRE(work_bytes >= sc_window_stats_workspace_bytes(a->n_win), "sc_window_stats: workspace too small (%zu < %zu bytes)", work_bytes,
             sc_window_stats_workspace_bytes(a->n_win));
  SC_REQUIRE((uintptr_t)work % 8 == 0, "sc_window_stats: workspace must be 8-byte aligned");
  const size_t n = (size_t)a->n_win;
  WsD d;
  d.x = a->x; d.rs = a->row_stride; d.H = a->H; d.W = a->W; d.n_win = a->n_win; d.nchunk = ws_chunks(a->n_win);
  d.win = a->windows; d.has_fill = a->has_fill ? 1 : 0; d.fill = a->fill; d.clip = a->clip_max;
  char* p = reinterpret_cast<char*>(work);
  d.st = reinterpret_cast<WsState*>(p); p += ws_align(n * sizeof(WsState));
  d.part = reinterpret_cast<WsPart*>(p); p += ws_align(n * d.nchunk * sizeof(WsPart));
  d.hist0 = reinterpret_cast<unsigned*>(p); p += ws_align(n * WS_BINS0 * sizeof(unsigned));
  d.hist = reinterpret_cast<unsigned*>(p);
  d.count = a->count; d.sum_mean = a->sum_mean; d.stats = a->stats;
  const int qs[4] = {1, 5, 95, 99};
  for (int j = 0; j < 4; ++j) d.q32[j] = (float)qs[j] / 100.0f;
  hipStream_t st = (hipStream_t)stream;
  // the picks leave the histograms zero, but the workspace is the caller's: it may be fresh or reused by something else
  const size_t hist_bytes = ws_align(n * WS_BINS0 * sizeof(unsigned)) + n * WS_R * WS_BINS * sizeof(unsigned);
  if (hipMemsetAsync(d.hist0, 0, hist_bytes, st) != hipSuccess) { sc_set_error("sc_window_stats: memset failed"); return SC_ERR_LAUNCH; }
  const dim3 gp((unsigned)(n * d.nchunk)), gk((unsigned)n), b(WS_WG);
  hipLaunchKernelGGL(k_ws_pass<0>, gp, b, 0, st, d);
  hipLaunchKernelGGL(k_ws_pick<0>, gk, b, 0, st, d);
  hipLaunchKernelGGL(k_ws_pass<1>, gp, b, 0, st, d);
  hipLaunchKernelGGL(k_ws_pick<1>, gk, b, 0, st, d);
  hipLaunchKernelGGL(k_ws_pass<2>, gp, b, 0, st, d);
  hipLaunchKernelGGL(k_ws_pick<2>, gk, b, 0, st, d);
  SC_LAUNCH_OK("sc_window_stats");
  return SC_OK;
}
