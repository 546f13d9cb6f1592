// Polygons -> label image (sc_rasterize_polygons): the inverse of sc_component_outlines, behind starcop_amd/plumes.py:
// rasterize_polygons.  include/starcop_hip.h states the rule (even-odd over all rings of a polygon, pixel centres, top-left ties,
// the later polygon wins); DESIGN section 26b argues it.
//   burn    : one wave per (polygon, row of its clipped box).  The lanes stride over the polygon's edges, apply the crossing test
//             at yc = r + 0.5 and compute the crossing abscissa xs in float64, every operation rounded on its own (contraction is
//             off for the whole file: numpy does not fuse, and the results are compared bit for bit).  A crossing toggles every
//             pixel from its first toggled column c_first on (the smallest c with c + 0.5 >= xs, found with exact comparisons), so
//             it is ONE bit: the lane flips bit c_first of a wave-private LDS bitmap of the box's columns (ds_xor, an integer
//             atomic: the order does not matter).  The inclusive prefix XOR of that bitmap is the parity of every column: 64 words
//             at a time, a shift cascade inside the 64-bit word, a ballot across the lanes, a carry across the groups.  Lane l then
//             writes bit l of every non-zero word: atomicMax(out + r*W + c, polygon index + 1), coalesced.  Integer max is
//             order-independent, so overlaps do not depend on scheduling and the later polygon wins.
//             There is no list of crossings, hence no cap on them: a row with any number of crossings costs the same bitmap.  A box
//             wider than the bitmap (RAST_CHUNK columns) is done in column chunks, the edges scanned once per chunk; a crossing left
//             of the chunk is clamped to its first column, which carries the parity in.
//   values  : only when the caller's values are not 1..P: one thread per pixel maps index + 1 -> values[index] in place.
// Work: sum over the polygons of box rows x (edges + box columns / 64).  Fine for plumes (hundreds of polygons, boxes of tens to
// hundreds of pixels), tolerable for a scene footprint (1e4 edges x 1e4 rows = 1e8 crossing tests); a sorted active-edge table
// would be the next step.  No work-group waits on another, no float atomics.
#pragma clang fp contract(off)
#include "sc_common.h"

namespace {

constexpr int RAST_WORDS = 1024;                 // 64-bit words of the bitmap: 8 KB of LDS per wave
constexpr int RAST_CHUNK = RAST_WORDS * 64;      // columns per pass over the edges
constexpr unsigned RAST_MAX_GRID = 1u << 20;

struct RastP {
  const double* edges; const sc_rast_poly* polys; int* out;
  int P, H, W; long long jobs;
};

// the polygon of a job: the last descriptor whose job0 <= job (job0 is non-decreasing; polygons without rows share a job0 with
// their successor and are never the last one at or below a job that exists)
__device__ __forceinline__ int poly_of(const sc_rast_poly* __restrict__ polys, int P, int job) {
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (polys[mid].job0 <= job) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(64) void k_rast_burn(const RastP p) {
  __shared__ unsigned long long bm[RAST_WORDS];
  unsigned* bm32 = reinterpret_cast<unsigned*>(bm);
  const int lane = threadIdx.x;
  for (long long job = blockIdx.x; job < p.jobs; job += gridDim.x) {
    const int i = poly_of(p.polys, p.P, (int)job);
    const sc_rast_poly d = p.polys[i];
    const int r = d.r0 + ((int)job - d.job0);
    if (r < d.r0 || r >= d.r1 || r >= p.H) continue;            // a table that is not the host's: write nothing
    const double yc = (double)r + 0.5;
    int* __restrict__ orow = p.out + (long long)r * p.W;
    for (int cb = d.c0; cb < d.c1; cb += RAST_CHUNK) {
      const int ce = min(d.c1, cb + RAST_CHUNK), nw = (ce - cb + 63) >> 6;
      for (int j = lane; j < nw; j += 64) bm[j] = 0ull;
      __syncthreads();                                          // one wave per work-group: orders its own LDS accesses
      const double lo = (double)cb + 0.5, hi = (double)(ce - 1) + 0.5;
      bool any = false;
      for (int e = d.e0 + lane; e < d.e1; e += 64) {
        const double2 a = reinterpret_cast<const double2*>(p.edges)[2 * (long long)e];
        const double2 b = reinterpret_cast<const double2*>(p.edges)[2 * (long long)e + 1];
        const double x0 = a.x, y0 = a.y, x1 = b.x, y1 = b.y;
        if ((y0 <= yc) == (y1 <= yc)) continue;
        const double t = yc - y0;
        const double dx = x1 - x0;
        const double m = t * dx;
        const double dy = y1 - y0;
        const double q = m / dy;
        const double xs = x0 + q;
        int cf;
        if (xs <= lo) cf = cb;                                  // toggles the whole chunk
        else if (!(xs <= hi)) continue;                         // first toggled column is right of the chunk
        else {
          cf = (int)xs;                                         // cb + 0.5 < xs <= ce - 0.5: in range, truncation = floor
          if (!((double)cf + 0.5 >= xs)) ++cf;
        }
        const int bit = cf - cb;
        atomicXor(&bm32[bit >> 5], 1u << (bit & 31));
        any = true;
      }
      if (!__any(any)) continue;                                // wave-uniform
      __syncthreads();
      unsigned carry = 0;
      for (int j0 = 0; j0 < nw; j0 += 64) {
        const int j = j0 + lane;
        unsigned long long w = j < nw ? bm[j] : 0ull;
        w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16; w ^= w << 32;       // bit k = parity of bits 0..k
        const unsigned long long odd = __ballot((w >> 63) != 0ull);
        const unsigned before = (unsigned)__popcll(odd & ((1ull << lane) - 1ull)) ^ carry;
        if (before & 1u) w = ~w;
        carry ^= (unsigned)__popcll(odd) & 1u;
        if (j < nw) bm[j] = w;
      }
      __syncthreads();
      for (int j = 0; j < nw; ++j) {
        const unsigned long long w = bm[j];                     // one address for the wave: a broadcast
        if (w == 0ull) continue;
        const int c = cb + j * 64 + lane;
        if (c < ce && ((w >> lane) & 1ull)) atomicMax(orow + c, i + 1);
      }
      __syncthreads();                                          // the bitmap is cleared again by the next chunk or job
    }
  }
}

__global__ __launch_bounds__(256) void k_rast_values(int* __restrict__ out, long long n, const int* __restrict__ values, int P) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int v = out[i];
  if (v > 0 && v <= P) out[i] = values[v - 1];
}

}  // namespace

extern "C" int sc_rasterize_polygons(const sc_rast_args* a, sc_stream stream) {
  SC_REQUIRE(a, "sc_rasterize_polygons: null arguments");
  SC_REQUIRE(a->H > 0 && a->W > 0 && (long long)a->H * a->W < (1ll << 31), "sc_rasterize_polygons: bad dims H=%d W=%d (H*W < 2^31)",
             a->H, a->W);
  SC_REQUIRE(a->out, "sc_rasterize_polygons: null out");
  SC_REQUIRE(a->P >= 0 && a->E >= 0 && a->E < (1ll << 31), "sc_rasterize_polygons: P=%d polygons, E=%lld edges (E < 2^31)", a->P,
             (long long)a->E);
  SC_REQUIRE(a->P == 0 || (a->polys && a->polys_host), "sc_rasterize_polygons: null polygon table (device and host)");
  SC_REQUIRE(a->E == 0 || (a->edges && ((uintptr_t)a->edges & 15) == 0), "sc_rasterize_polygons: edges null or not 16-byte aligned");
  long long jobs = 0;
  for (int i = 0; i < a->P; ++i) {
    const sc_rast_poly& d = a->polys_host[i];
    SC_REQUIRE(d.e0 >= 0 && d.e0 <= d.e1 && d.e1 <= a->E, "sc_rasterize_polygons: polygon %d: edges [%d, %d) of %lld", i, d.e0, d.e1,
               (long long)a->E);
    SC_REQUIRE(d.r0 >= 0 && d.r0 <= d.r1 && d.r1 <= a->H && d.c0 >= 0 && d.c0 <= d.c1 && d.c1 <= a->W,
               "sc_rasterize_polygons: polygon %d: box rows [%d, %d) columns [%d, %d) leaves the %d x %d raster", i, d.r0, d.r1, d.c0,
               d.c1, a->H, a->W);
    SC_REQUIRE(d.job0 == jobs, "sc_rasterize_polygons: polygon %d: job0 %d, expected %lld (the running sum of the box rows)", i, d.job0,
               jobs);
    if (d.c1 > d.c0 && d.e1 > d.e0) jobs += d.r1 - d.r0;
    SC_REQUIRE(jobs < (1ll << 31), "sc_rasterize_polygons: more than 2^31 - 1 (polygon, row) jobs");
  }
  hipStream_t st = (hipStream_t)stream;
  const long long HW = (long long)a->H * a->W;
  if (hipMemsetAsync(a->out, 0, (size_t)HW * 4, st) != hipSuccess) {
    sc_set_error("sc_rasterize_polygons: hipMemsetAsync failed");
    return SC_ERR_LAUNCH;
  }
  if (jobs == 0) return SC_OK;
  RastP p{a->edges, a->polys, a->out, a->P, a->H, a->W, jobs};
  const unsigned grid = (unsigned)(jobs < (long long)RAST_MAX_GRID ? jobs : (long long)RAST_MAX_GRID);
  hipLaunchKernelGGL(k_rast_burn, dim3(grid), dim3(64), 0, st, p);
  SC_LAUNCH_OK("k_rast_burn");
  if (a->values) {
    hipLaunchKernelGGL(k_rast_values, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, st, a->out, HW, a->values, a->P);
    SC_LAUNCH_OK("k_rast_values");
  }
  return SC_OK;
}
