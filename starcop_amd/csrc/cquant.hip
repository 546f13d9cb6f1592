// Exact order statistics per labelled component (sc_component_quantiles): the ring median, the MAD and the plume percentiles
// behind starcop_amd/plumes.py: component_quantiles.  Component k of image n is the set of pixels of value k, 1 <= k <=
// min(counts[n], M); its members are the pixels whose value t (the plane value v, or |v - center| of its row) is finite.
//   count   : one work-group per 2048 pixels; members are counted per row, first in a table in LDS, then with one integer atomic
//             per work-group and row in it.
//   plan    : one thread per row.  Every row takes a contiguous segment of the key buffer (a wave-wide prefix sum and one
//             atomic add per wave on the running total: which segment a row gets depends on arrival, what it holds does not).
//             A row of more than SC_CQUANT_SMALL_MAX members registers as a large segment: a state record with its ranks and
//             one work item per 4096 keys.
//   scatter : the count pass again; every member stores its key at segment + slot, the slot from the same atomics.  Keys are the
//             monotone map of the float bits (sign bit flipped for non-negatives, all bits inverted for negatives), so unsigned
//             order is value order for both signs.  The order inside a segment is arbitrary and does not matter.
//   tiny    : one wave per row.  Writes n_finite of every row and NaN for n = 0 (and rows at or above counts[n]); a row of at
//             most 64 members is sorted by a bitonic network over the lanes (shuffles only) and its ranks are read off.
//   small   : one work-group per row of 65 .. SC_CQUANT_SMALL_MAX members: the segment is loaded into LDS, padded to a power of
//             two with the largest key, sorted by a bitonic network and the ranks are read off.
//   large   : four passes of an 8-bit radix select over the contiguous keys of the large segments, all 2 Q ranks of a segment
//             together (the scheme of winstats.hip): `hist` counts, per work item, the digit of every key whose higher digits
//             equal one of the segment's distinct rank prefixes (LDS histogram, then integer atomics into the segment's own);
//             `pick` scans the 256 bins, moves every rank into its bin and groups the ranks by their new prefix.
// Selection is exact and only integer atomics are used, so the result does not depend on the order in which values arrive:
// repeated calls, and an image alone or in a batch, give identical bytes.  Interpolation: numpy >= 2.0 on float32 data, every
// operation rounded to float32 and none fused (np_lerp as in winstats.hip).
#include "sc_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int MAXQ = SC_CQUANT_MAX_Q;
constexpr int MAXR = 2 * MAXQ;                  // ranks per row: two neighbours per quantile
constexpr int SMALL = SC_CQUANT_SMALL_MAX;
constexpr int CHUNK = 4096;                     // keys per work item of the large path
constexpr int BINS = 256;
constexpr unsigned PAD_KEY = 0xffffffffu;       // above the key of every finite value (the largest is 0xff7fffff)

struct Hdr { unsigned total, nlarge, nitems, pad; };
struct LState {
  unsigned row, n, off;
  int nslot;
  unsigned k[MAXR], prefix[MAXR], slot_prefix[MAXR];
  int rank_slot[MAXR];
};

struct CqP {
  const int* labels; const int* counts; const float* plane; long long plane_stride; const float* center;
  int N, H, W, M, Q;
  float q[MAXQ];
  long long* n_finite; float* quantile;
  Hdr* hdr;
  unsigned* cnt;                                // [N*M] members per row
  unsigned* cursor;                             // [N*M] next free slot of the row's segment
  unsigned* hist0;                              // [maxL][256] first-pass histograms
  unsigned* off;                                // [N*M] first key of the row's segment
  unsigned* keys;                               // [N*H*W]
  LState* ls;                                   // [maxL]
  uint2* items;                                 // [maxI] (large segment, chunk)
  unsigned* hist;                               // [maxL][MAXR][256] histograms of passes 1 .. 3
  unsigned maxL, maxI;
};

__device__ __forceinline__ int n_components(const CqP& p, int n) { return min(max(p.counts[n], 0), p.M); }
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// is pixel i of image n a member, of which row and with which key
__device__ __forceinline__ bool member(const CqP& p, int n, long long i, int ncomp, unsigned& row, unsigned& key) {
  const int k = p.labels[(size_t)n * p.H * p.W + i];
  if (k < 1 || k > ncomp) return false;                            // background, and values that name no row
  row = (unsigned)n * (unsigned)p.M + (unsigned)(k - 1);
  float t = p.plane[(long long)n * p.plane_stride + i];
  if (p.center) t = fabsf(t - p.center[row]);
  key = key_of(t);
  return finite_f(t);
}

// Both gather passes: ctr[row] += 1 for every member, and with SCATTER the member's key stored at off[row] + (the value before its
// add).  One work-group takes GATHER_PX consecutive pixels.  Members are first counted in a small table in LDS, hashed by row
// (a slot is claimed by compare-and-swap; a member whose slot belongs to another row adds to the global counter on its own), then
// ONE global atomic per used slot reserves the rows' ranges, and the members take their places inside them.  A component that
// covers much of the image then costs one global atomic per work-group, not one per wave: adds on one address are served one
// after the other.  Integer adds only: counters and slots come out disjoint in any order.
constexpr int GATHER_STEPS = 8, GATHER_PX = 256 * GATHER_STEPS, GATHER_SLOTS = 128;
constexpr unsigned NO_ROW = 0xffffffffu;

template <bool SCATTER>
__global__ __launch_bounds__(256) void k_cq_gather(const CqP p) {
  __shared__ unsigned h_row[GATHER_SLOTS], h_cnt[GATHER_SLOTS], h_base[GATHER_SLOTS];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long HW = (long long)p.H * p.W, first = (long long)blockIdx.x * GATHER_PX;
  unsigned* ctr = SCATTER ? p.cursor : p.cnt;
  if (tid < GATHER_SLOTS) { h_row[tid] = NO_ROW; h_cnt[tid] = 0; }
  __syncthreads();
  const int ncomp = n_components(p, n);
  unsigned row[GATHER_STEPS], key[GATHER_STEPS], slot[GATHER_STEPS];
  unsigned act = 0, cached = 0;                                    // one bit per step
#pragma unroll
  for (int s = 0; s < GATHER_STEPS; ++s) {
    const long long i = first + s * 256 + tid;
    row[s] = 0; key[s] = 0; slot[s] = 0;
    if (i < HW && member(p, n, i, ncomp, row[s], key[s])) {
      act |= 1u << s;
      const unsigned e = row[s] & (GATHER_SLOTS - 1);
      const unsigned owner = atomicCAS(&h_row[e], NO_ROW, row[s]);
      if (owner == NO_ROW || owner == row[s]) {
        cached |= 1u << s;
        slot[s] = atomicAdd(&h_cnt[e], 1u);
      } else {
        slot[s] = atomicAdd(ctr + row[s], 1u);
      }
    }
  }
  __syncthreads();
  if (tid < GATHER_SLOTS && h_cnt[tid]) h_base[tid] = atomicAdd(ctr + h_row[tid], h_cnt[tid]);
  if (!SCATTER) return;
  __syncthreads();
#pragma unroll
  for (int s = 0; s < GATHER_STEPS; ++s) {
    if (!(act >> s & 1u)) continue;
    const unsigned at = (cached >> s & 1u) ? h_base[row[s] & (GATHER_SLOTS - 1)] + slot[s] : slot[s];
    p.keys[(size_t)p.off[row[s]] + at] = key[s];
  }
}

// the two ranks of quantile q among n >= 1 members: a negative q is the median
__device__ __forceinline__ void ranks_of(unsigned n, float q, unsigned& lo, unsigned& hi) {
  if (q < 0.f) { lo = (n - 1u) / 2u; hi = n / 2u; return; }
  const float vi = (float)(n - 1u) * q;
  lo = min((unsigned)floorf(vi), n - 1u);
  hi = min(lo + 1u, n - 1u);
}
// numpy's _lerp on float32 operands: every operation rounds to float32, none is fused
__device__ __forceinline__ float np_lerp(float a, float b, float t) {
  const float d = b - a;
  float r = a + d * t;
  if (t >= 0.5f) r = b - d * (1.0f - t);
  return r;
}
__device__ __forceinline__ float quantile_of(unsigned n, float q, float a, float b) {
  if (q < 0.f) return (a + b) / 2.0f;
  const float vi = (float)(n - 1u) * q;
  return np_lerp(a, b, n > 1u ? vi - floorf(vi) : 0.f);
}

__global__ __launch_bounds__(256) void k_cq_plan(const CqP p) {
  const long long rows = (long long)p.N * p.M;
  const long long r64 = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = r64 < rows;
  const unsigned row = live ? (unsigned)r64 : 0u;
  const unsigned c = live ? p.cnt[row] : 0u;
  unsigned incl = c;                                               // the sum of all counts is below 2^32: one per pixel
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  unsigned base = 0;
  if (lane == 63 && incl) base = atomicAdd(&p.hdr->total, incl);
  base = __shfl(base, 63, 64);
  if (!live) return;
  const unsigned off = base + incl - c;
  p.off[row] = off;
  if (c <= (unsigned)SMALL) return;
  const unsigned sl = atomicAdd(&p.hdr->nlarge, 1u);
  if (sl >= p.maxL) return;                                        // cannot happen: more than SMALL pixels each
  LState& s = p.ls[sl];
  s.row = row; s.n = c; s.off = off; s.nslot = 1;
  for (int r = 0; r < MAXR; ++r) { s.k[r] = 0; s.prefix[r] = 0; s.slot_prefix[r] = 0; s.rank_slot[r] = 0; }
  for (int j = 0; j < p.Q; ++j) ranks_of(c, p.q[j], s.k[2 * j], s.k[2 * j + 1]);
  const unsigned nch = (c + CHUNK - 1) / CHUNK;
  const unsigned ib = atomicAdd(&p.hdr->nitems, nch);
  for (unsigned j = 0; j < nch && ib + j < p.maxI; ++j) p.items[ib + j] = make_uint2(sl, j);
}

// rows of at most 64 members, one wave each: n_finite of every row, NaN for the empty ones, a bitonic network over the lanes
__global__ __launch_bounds__(256) void k_cq_tiny(const CqP p) {
  const long long r64 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r64 >= (long long)p.N * p.M) return;                         // whole waves leave together
  const unsigned row = (unsigned)r64;
  const int lane = threadIdx.x & 63;
  const int n_img = (int)(row / (unsigned)p.M), m = (int)(row - (unsigned)n_img * (unsigned)p.M);
  const unsigned n = m < n_components(p, n_img) ? p.cnt[row] : 0u;  // the same in every lane
  if (lane == 0) p.n_finite[row] = n;
  float* out = p.quantile + (size_t)row * p.Q;
  if (n == 0) {
    if (lane < p.Q) out[lane] = __builtin_nanf("");
    return;
  }
  if (n > 64u) return;
  unsigned v = (unsigned)lane < n ? p.keys[(size_t)p.off[row] + lane] : PAD_KEY;
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const unsigned o = __shfl_xor(v, j, 64);
      v = (((lane & j) == 0) == ((lane & k) == 0)) ? min(v, o) : max(v, o);
    }
  }
  unsigned lo = 0, hi = 0;
  const float q = p.q[lane < p.Q ? lane : 0];
  ranks_of(n, q, lo, hi);
  const unsigned a = __shfl(v, (int)lo, 64), b = __shfl(v, (int)hi, 64);
  if (lane < p.Q) out[lane] = quantile_of(n, q, value_of(a), value_of(b));
}

__global__ __launch_bounds__(256) void k_cq_small(const CqP p) {
  __shared__ unsigned s[SMALL];
  const unsigned row = blockIdx.x, tid = threadIdx.x;
  const int n_img = (int)(row / (unsigned)p.M), m = (int)(row - (unsigned)n_img * (unsigned)p.M);
  const unsigned n = m < n_components(p, n_img) ? p.cnt[row] : 0u;
  if (n <= 64u || n > (unsigned)SMALL) return;                     // k_cq_tiny and the large path write those
  float* out = p.quantile + (size_t)row * p.Q;
  unsigned P = 2;
  while (P < n) P <<= 1;
  const unsigned* kb = p.keys + p.off[row];
  for (unsigned i = tid; i < P; i += 256) s[i] = i < n ? kb[i] : PAD_KEY;
  __syncthreads();
  for (unsigned k = 2; k <= P; k <<= 1) {
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      for (unsigned t = tid; t < P / 2; t += 256) {
        const unsigned i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
        const unsigned a = s[i], b = s[l];
        if ((a > b) == ((i & k) == 0u)) { s[i] = b; s[l] = a; }
      }
      __syncthreads();
    }
  }
  if ((int)tid < p.Q) {
    unsigned lo, hi;
    ranks_of(n, p.q[tid], lo, hi);
    out[tid] = quantile_of(n, p.q[tid], value_of(s[lo]), value_of(s[hi]));
  }
}

// digit of pass PASS (0: the top eight bits) and the digits above it
template <int PASS> __device__ __forceinline__ unsigned digit_of(unsigned key) { return (key >> (24 - 8 * PASS)) & 255u; }
template <int PASS> __device__ __forceinline__ unsigned high_of(unsigned key) { return PASS == 0 ? 0u : key >> (32 - 8 * PASS); }

template <int PASS>
__global__ __launch_bounds__(256) void k_cq_hist(const CqP p) {
  __shared__ unsigned h[(PASS == 0 ? 1 : MAXR) * BINS];
  __shared__ unsigned s_pre[MAXR];
  if (blockIdx.x >= min(p.hdr->nitems, p.maxI)) return;
  const uint2 it = p.items[blockIdx.x];
  const unsigned tid = threadIdx.x;
  const LState& st = p.ls[it.x];
  const int nslot = PASS == 0 ? 1 : min(max(st.nslot, 0), MAXR);
  if (tid < (unsigned)MAXR) s_pre[tid] = st.slot_prefix[tid];
  for (unsigned i = tid; i < (unsigned)nslot * BINS; i += 256) h[i] = 0;
  __syncthreads();
  const unsigned first = it.y * CHUNK, last = min(st.n, first + CHUNK);
  const unsigned* kb = p.keys + st.off;
  for (unsigned i = first + tid; i < last; i += 256) {
    const unsigned key = kb[i], hi = high_of<PASS>(key);
    for (int sl = 0; sl < nslot; ++sl)
      if (s_pre[sl] == hi) { atomicAdd(&h[sl * BINS + digit_of<PASS>(key)], 1u); break; }      // the prefixes are distinct
  }
  __syncthreads();
  unsigned* g = PASS == 0 ? p.hist0 + (size_t)it.x * BINS : p.hist + (size_t)it.x * MAXR * BINS;
  for (unsigned i = tid; i < (unsigned)nslot * BINS; i += 256)
    if (h[i]) atomicAdd(g + i, h[i]);
}

// One work-group per large segment, one thread per bin.  For every histogram in use an exclusive scan over its bins; the thread
// whose bin holds rank k of an order statistic records the digit.  Leaves the histograms of the next pass zeroed.
template <int PASS>
__global__ __launch_bounds__(256) void k_cq_pick(const CqP p) {
  __shared__ unsigned scan[2][BINS];
  __shared__ unsigned new_prefix[MAXR], new_k[MAXR];
  __shared__ LState s;
  if (blockIdx.x >= min(p.hdr->nlarge, p.maxL)) return;
  const unsigned t = threadIdx.x;
  const int R = 2 * p.Q;
  if (t == 0) s = p.ls[blockIdx.x];
  if (t < (unsigned)MAXR) { new_prefix[t] = 0; new_k[t] = 0; }
  __syncthreads();
  const int nslot = PASS == 0 ? 1 : min(max(s.nslot, 0), MAXR);
  unsigned* g = PASS == 0 ? p.hist0 + (size_t)blockIdx.x * BINS : p.hist + (size_t)blockIdx.x * MAXR * BINS;
  for (int sl = 0; sl < nslot; ++sl) {
    const unsigned c = g[sl * BINS + t];
    int cur = 0;
    scan[0][t] = c;
    __syncthreads();
    for (unsigned o = 1; o < (unsigned)BINS; o <<= 1) {
      scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0u);
      cur ^= 1;
      __syncthreads();
    }
    const unsigned before = scan[cur][t] - c;                      // keys in the lower bins
    for (int r = 0; r < R; ++r) {
      if (s.rank_slot[r] != sl) continue;
      const unsigned k = s.k[r];
      if (k >= before && k - before < c) { new_prefix[r] = (s.prefix[r] << 8) | t; new_k[r] = k - before; }
    }
    __syncthreads();
  }
  if (PASS < 3) {
    unsigned* z = p.hist + (size_t)blockIdx.x * MAXR * BINS;       // each thread read its own bins only
    for (int sl = 0; sl < MAXR; ++sl) z[sl * BINS + t] = 0;
    if (t != 0) return;
    int ns = 0;                                                    // the distinct prefixes of the ranks: one histogram each
    for (int r = 0; r < R; ++r) {
      s.prefix[r] = new_prefix[r];
      s.k[r] = new_k[r];
      int sl = -1;
      for (int q = 0; q < ns; ++q)
        if (s.slot_prefix[q] == new_prefix[r]) sl = q;
      if (sl < 0) { sl = ns; s.slot_prefix[ns++] = new_prefix[r]; }
      s.rank_slot[r] = sl;
    }
    s.nslot = ns;
    p.ls[blockIdx.x] = s;
  } else if ((int)t < p.Q) {
    p.quantile[(size_t)s.row * p.Q + t] = quantile_of(s.n, p.q[t], value_of(new_prefix[2 * t]), value_of(new_prefix[2 * t + 1]));
  }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
bool dims_ok(int N, int H, int W, int M, int Q) {
  return N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W < (1ll << 31) && (long long)N * H * W < (1ll << 32) && M >= 0 &&
         (long long)N * M < (1ll << 31) && Q >= 1 && Q <= MAXQ;
}
struct Layout {
  size_t rows, px, maxL, maxI;
  size_t cnt, cursor, hist0, zero_end, off, keys, ls, items, hist, total;
};
Layout layout_of(int N, int H, int W, int M) {
  Layout l{};
  l.rows = (size_t)N * M;
  l.px = (size_t)N * H * W;
  l.maxL = l.px / (SMALL + 1) < l.rows ? l.px / (SMALL + 1) : l.rows;     // segments of more than SMALL keys
  l.maxI = l.px / CHUNK + l.maxL;                                  // sum of ceil(n / CHUNK) over them
  size_t at = align256(sizeof(Hdr));
  l.cnt = at; at += align256(l.rows * 4);
  l.cursor = at; at += align256(l.rows * 4);
  l.hist0 = at; at += align256(l.maxL * BINS * 4);
  l.zero_end = at;                                                 // everything up to here is cleared at the start of a call
  l.off = at; at += align256(l.rows * 4);
  l.keys = at; at += align256(l.px * 4);
  l.ls = at; at += align256(l.maxL * sizeof(LState));
  l.items = at; at += align256(l.maxI * sizeof(uint2));
  l.hist = at; at += align256(l.maxL * MAXR * BINS * 4);
  l.total = at;
  return l;
}

}  // namespace

extern "C" size_t sc_component_quantiles_workspace_bytes(int N, int H, int W, int M, int Q) {
  if (!dims_ok(N, H, W, M, Q)) return 0;
  return layout_of(N, H, W, M).total;
}

extern "C" int sc_component_quantiles(const sc_cquant_args* a, void* work, size_t work_bytes, sc_stream stream) {
  SC_REQUIRE(a, "sc_component_quantiles: null arguments");
  SC_REQUIRE(dims_ok(a->N, a->H, a->W, a->M, a->Q),
             "sc_component_quantiles: bad dims N=%d H=%d W=%d M=%d Q=%d (N <= 65535, H*W < 2^31, N*H*W < 2^32, N*M < 2^31, 1 <= Q <= %d)",
             a->N, a->H, a->W, a->M, a->Q, MAXQ);
  for (int j = 0; j < a->Q; ++j)
    SC_REQUIRE(a->q[j] <= 1.0f, "sc_component_quantiles: q[%d] = %g (a fraction in [0, 1], or negative for the median)", j,
               (double)a->q[j]);                                   // NaN fails the comparison
  SC_REQUIRE(a->labels && a->counts && a->plane, "sc_component_quantiles: null labels, counts or plane");
  SC_REQUIRE(a->N == 1 || a->plane_stride >= (long long)a->H * a->W, "sc_component_quantiles: plane stride %lld overlaps %d x %d images",
             (long long)a->plane_stride, a->H, a->W);
  const Layout l = layout_of(a->N, a->H, a->W, a->M);
  SC_REQUIRE(work && work_bytes >= l.total, "sc_component_quantiles: workspace %zu < %zu bytes", work_bytes, l.total);
  if (a->M == 0) return SC_OK;                                      // no rows to write
  SC_REQUIRE(a->n_finite && a->quantile, "sc_component_quantiles: null output column");
  hipStream_t st = (hipStream_t)stream;
  char* wp = static_cast<char*>(work);
  CqP p{};
  p.labels = a->labels; p.counts = a->counts; p.plane = a->plane; p.plane_stride = a->plane_stride; p.center = a->center;
  p.N = a->N; p.H = a->H; p.W = a->W; p.M = a->M; p.Q = a->Q;
  for (int j = 0; j < a->Q; ++j) p.q[j] = a->q[j];
  p.n_finite = (long long*)a->n_finite; p.quantile = a->quantile;
  p.hdr = reinterpret_cast<Hdr*>(wp);
  p.cnt = reinterpret_cast<unsigned*>(wp + l.cnt); p.cursor = reinterpret_cast<unsigned*>(wp + l.cursor);
  p.hist0 = reinterpret_cast<unsigned*>(wp + l.hist0); p.off = reinterpret_cast<unsigned*>(wp + l.off);
  p.keys = reinterpret_cast<unsigned*>(wp + l.keys); p.ls = reinterpret_cast<LState*>(wp + l.ls);
  p.items = reinterpret_cast<uint2*>(wp + l.items); p.hist = reinterpret_cast<unsigned*>(wp + l.hist);
  p.maxL = (unsigned)l.maxL; p.maxI = (unsigned)l.maxI;
  if (hipMemsetAsync(wp, 0, l.zero_end, st) != hipSuccess) {
    sc_set_error("sc_component_quantiles: clearing the counters failed");
    return SC_ERR_LAUNCH;
  }
  const dim3 px((unsigned)(((long long)a->H * a->W + GATHER_PX - 1) / GATHER_PX), a->N), rows((unsigned)((l.rows + 255) / 256));
  hipLaunchKernelGGL(k_cq_gather<false>, px, dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cq_gather<count>");
  hipLaunchKernelGGL(k_cq_plan, rows, dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cq_plan");
  hipLaunchKernelGGL(k_cq_gather<true>, px, dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cq_gather<scatter>");
  hipLaunchKernelGGL(k_cq_tiny, dim3((unsigned)((l.rows + 3) / 4)), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cq_tiny");
  if (l.px <= 64) return SC_OK;                                     // no row can hold more than a wave
  hipLaunchKernelGGL(k_cq_small, dim3((unsigned)l.rows), dim3(256), 0, st, p);
  SC_LAUNCH_OK("k_cq_small");
  if (l.maxL == 0) return SC_OK;                                    // no image can hold a large segment
  const dim3 gi((unsigned)l.maxI), gl((unsigned)l.maxL);
#define CQ_PASS(P)                                                  \
  hipLaunchKernelGGL(k_cq_hist<P>, gi, dim3(256), 0, st, p);        \
  SC_LAUNCH_OK("k_cq_hist");                                        \
  hipLaunchKernelGGL(k_cq_pick<P>, gl, dim3(256), 0, st, p);        \
  SC_LAUNCH_OK("k_cq_pick");
  CQ_PASS(0) CQ_PASS(1) CQ_PASS(2) CQ_PASS(3)
#undef CQ_PASS
  return SC_OK;
}
