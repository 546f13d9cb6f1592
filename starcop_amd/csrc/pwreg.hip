// Pointwise regression networks (SimpleCNN_v2: one 1x1 convolution, SimpleCNN_v3: two with no activation between them):
// forward, L1 / MSE loss, and the fused training sweep whose two moments give every parameter gradient ("Regression
// path").  Reference lines are cited at each entry point in include/starcop_hip.h.
#include "sc_common.h"

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int PW_C = SC_PWREG_MAXC;           // 16: channel limit = one MFMA tile
constexpr int PW_TILE = 128;                  // pixels of one wave per sweep iteration (two per lane)
constexpr int PW_LD = 132;                    // floats between two channel rows of a staged tile: 16-byte aligned, and the 16 rows x 4
                                              // quarter-rows one MFMA operand read touches fall on distinct LDS banks
constexpr int PW_WF = 2 * (PW_C * PW_C + PW_C);   // zero-padded weights in LDS: W1[16][16] b1[16] W2[16][16] b2[16]
constexpr int PW_ROW = SC_PWREG_PART_DOUBLES;     // one partial row: M[16][16], s[16], loss
constexpr int PW_MAX_BLOCKS = 512;
constexpr int PW_FIN_THREADS = 1024;

struct PwDims { int Cin, C1, Cout, layers; };

// flat parameters (state_dict order) -> the zero-padded LDS image; all threads of the block, followed by a barrier at the caller
__device__ __forceinline__ void pw_stage_weights(const float* __restrict__ params, PwDims d, float* sW) {
  for (int i = threadIdx.x; i < PW_WF; i += blockDim.x) sW[i] = 0.f;
  __syncthreads();
  const int n1 = d.C1 * d.Cin;
  for (int i = threadIdx.x; i < n1; i += blockDim.x) sW[(i / d.Cin) * PW_C + i % d.Cin] = params[i];
  for (int i = threadIdx.x; i < d.C1; i += blockDim.x) sW[PW_C * PW_C + i] = params[n1 + i];
  if (d.layers == 2) {
    const float* p2 = params + n1 + d.C1;
    const int n2 = d.Cout * d.C1;
    float* s2 = sW + PW_C * PW_C + PW_C;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) s2[(i / d.C1) * PW_C + i % d.C1] = p2[i];
    for (int i = threadIdx.x; i < d.Cout; i += blockDim.x) s2[PW_C * PW_C + i] = p2[n2 + i];
  }
}

// one 1x1 layer on V pixels of a lane: out[o] = b[o] + sum_i W[o][i] in[i], an fp32 fmaf chain in ascending i (the padded terms
// add +0 exactly).  nin / nout are wave-uniform, the loops are unrolled so that every register index is static.
template <int V>
__device__ __forceinline__ void pw_layer(const float* W, const float* b, int nin, int nout, const float (&in)[PW_C][V],
                                         float (&out)[PW_C][V]) {
#pragma unroll
  for (int o = 0; o < PW_C; ++o) {
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    if (o < nout) {
      const float bo = b[o];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = bo;
#pragma unroll
      for (int i4 = 0; i4 < PW_C / 4; ++i4) {
        if (4 * i4 < nin) {
          const float4 w = *reinterpret_cast<const float4*>(W + o * PW_C + 4 * i4);
#pragma unroll
          for (int v = 0; v < V; ++v) {
            acc[v] = fmaf(w.x, in[4 * i4 + 0][v], acc[v]);
            acc[v] = fmaf(w.y, in[4 * i4 + 1][v], acc[v]);
            acc[v] = fmaf(w.z, in[4 * i4 + 2][v], acc[v]);
            acc[v] = fmaf(w.w, in[4 * i4 + 3][v], acc[v]);
          }
        }
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) out[o][v] = acc[v];
  }
}

template <int V>
__device__ __forceinline__ void pw_eval(const float* sW, PwDims d, const float (&x)[PW_C][V], float (&p)[PW_C][V]) {
  if (d.layers == 2) {
    float h[PW_C][V];
    pw_layer<V>(sW, sW + PW_C * PW_C, d.Cin, d.C1, x, h);
    pw_layer<V>(sW + PW_C * PW_C + PW_C, sW + 2 * PW_C * PW_C + PW_C, d.C1, d.Cout, h, p);
  } else {
    pw_layer<V>(sW, sW + PW_C * PW_C, d.Cin, d.C1, x, p);
  }
}

// V pixels p0 .. p0+V-1 of nch planes of one image (`img` = its first plane); pixels >= HW and channels >= nch read as 0.
// VEC: every plane starts on a V*4-byte boundary and HW is a multiple of V, so a lane's V pixels are one aligned load.  (A template
// parameter, not a run-time flag: with a flag the compiler merges the two paths into element loads.)
template <int V, bool VEC>
__device__ __forceinline__ void pw_load(const float* __restrict__ img, size_t HW, int nch, size_t p0, float (&r)[PW_C][V]) {
#pragma unroll
  for (int c = 0; c < PW_C; ++c) {
#pragma unroll
    for (int v = 0; v < V; ++v) r[c][v] = 0.f;
    if (c < nch) {
      const float* q = img + (size_t)c * HW + p0;
      if constexpr (VEC) {
        if (p0 < HW) {
          if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(q);
            r[c][0] = t.x; r[c][1] = t.y; r[c][2] = t.z; r[c][3] = t.w;
          } else {
            const float2 t = *reinterpret_cast<const float2*>(q);
            r[c][0] = t.x; r[c][1] = t.y;
          }
        }
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v)
          if (p0 + v < HW) r[c][v] = q[v];
      }
    }
  }
}

// ---------------------------------------------------------------- forward
template <bool VEC>
__global__ __launch_bounds__(256) void k_pwreg_fwd(const float* __restrict__ x, const float* __restrict__ params, PwDims d, size_t HW,
                                                   float* __restrict__ pred) {
  __shared__ __attribute__((aligned(16))) float sW[PW_WF];
  pw_stage_weights(params, d, sW);
  __syncthreads();
  const size_t n = blockIdx.y;
  const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= HW) return;
  float xr[PW_C][4], p[PW_C][4];
  pw_load<4, VEC>(x + n * d.Cin * HW, HW, d.Cin, p0, xr);
  pw_eval<4>(sW, d, xr, p);
  float* o = pred + n * d.Cout * HW + p0;
#pragma unroll
  for (int c = 0; c < PW_C; ++c) {
    if (c < d.Cout) {
      float* q = o + (size_t)c * HW;
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(q) = make_float4(p[c][0], p[c][1], p[c][2], p[c][3]);
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (p0 + v < HW) q[v] = p[c][v];
      }
    }
  }
}

// ---------------------------------------------------------------- loss
// per-block fp64 partial of sum |d| (L1) or sum d^2 (MSE), d = pred - y, and optionally dL/dpred of the MEAN; fixed grid-stride
// assignment and a fixed summation order: repeated calls give identical bits
template <int KIND>
__global__ __launch_bounds__(256) void k_reg_loss(const float* __restrict__ pred, const float* __restrict__ y, size_t n, float inv_n,
                                                  float* __restrict__ dpred, double* __restrict__ part) {
  __shared__ double s_tmp[4];
  double acc = 0.0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float dlt = pred[i] - y[i];
    if (KIND == SC_REG_L1) {
      acc += (double)fabsf(dlt);
      if (dpred) dpred[i] = dlt > 0.f ? inv_n : (dlt < 0.f ? -inv_n : dlt);       // sign(0) = 0 (and NaN stays NaN) as torch has it
    } else {
      acc += (double)dlt * (double)dlt;
      if (dpred) dpred[i] = 2.f * dlt * inv_n;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  acc = wave_sum_d(acc);
  if (lane == 0) s_tmp[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((s_tmp[0] + s_tmp[1]) + s_tmp[2]) + s_tmp[3];
}

__global__ __launch_bounds__(64) void k_reg_loss_sum(const double* __restrict__ part, int nparts, double* __restrict__ loss_sum) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 64) acc += part[i];
  acc = wave_sum_d(acc);
  if (threadIdx.x == 0) loss_sum[0] = acc;
}

// ---------------------------------------------------------------- fused training sweep
// MODE SC_REG_L1 / SC_REG_MSE: g = sign(pred - y) or (pred - y) from x and y in registers (the factor 1/n or 2/n is applied in fp64
// by the finalize); MODE SC_PWREG_G_FROM_MEMORY: g is read from `yg`.  Each wave stages its 128 pixels of x and g as channel rows in
// LDS and accumulates M = sum g x^T on v_mfma_f64_16x16x4_f64: lane l feeds A[l & 15][l >> 4] = g[channel l & 15] and
// B[l >> 4][l & 15] = x[channel l & 15] of the same pixel, so the k index only has to name the same pixel on both sides.  With
// Cin < 16 column Cin of B is the constant 1 and collects s = sum g; with Cin == 16 a second accumulator against B = 1 does.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void k_pwreg_sweep(const float* __restrict__ x, const float* __restrict__ yg,
                                                     const float* __restrict__ params, PwDims d, size_t HW, int tiles_per_img,
                                                     long long ntiles, int iters, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sW = smem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* sX = smem + PW_WF + (size_t)wave * (d.Cin + d.Cout) * PW_LD;
  float* sG = sX + (size_t)d.Cin * PW_LD;
  if (MODE != SC_PWREG_G_FROM_MEMORY) pw_stage_weights(params, d, sW);
  __syncthreads();

  const int r = lane & 15, q = lane >> 4;
  doublex4 accM = {0.0, 0.0, 0.0, 0.0}, accS = {0.0, 0.0, 0.0, 0.0};
  double loss = 0.0;
  const bool ones_col = d.Cin < PW_C;
  for (int it = 0; it < iters; ++it) {
    const long long t = (long long)it * gridDim.x * 4 + (long long)blockIdx.x * 4 + wave;
    const bool live = t < ntiles;
    const size_t n = live ? (size_t)(t / tiles_per_img) : 0;
    const size_t p0 = live ? (size_t)(t % tiles_per_img) * PW_TILE + 2 * lane : HW;      // p0 >= HW: everything below is masked to 0
    float xr[PW_C][2], g[PW_C][2];
    pw_load<2, VEC>(x + n * d.Cin * HW, HW, d.Cin, p0, xr);
    pw_load<2, VEC>(yg + n * d.Cout * HW, HW, d.Cout, p0, g);                             // y, or g itself
    if (MODE != SC_PWREG_G_FROM_MEMORY) {
      float p[PW_C][2];
      pw_eval<2>(sW, d, xr, p);
#pragma unroll
      for (int c = 0; c < PW_C; ++c) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const bool in = c < d.Cout && p0 + v < HW;
          const float dlt = in ? p[c][v] - g[c][v] : 0.f;
          if (MODE == SC_REG_L1) {
            loss += (double)fabsf(dlt);
            g[c][v] = dlt > 0.f ? 1.f : (dlt < 0.f ? -1.f : dlt);
          } else {
            loss += (double)dlt * (double)dlt;
            g[c][v] = dlt;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < PW_C; ++c) {
      if (c < d.Cin) *reinterpret_cast<float2*>(sX + c * PW_LD + 2 * lane) = make_float2(xr[c][0], xr[c][1]);
      if (c < d.Cout) *reinterpret_cast<float2*>(sG + c * PW_LD + 2 * lane) = make_float2(g[c][0], g[c][1]);
    }
    __syncthreads();
    const bool a_on = r < d.Cout, b_on = r < d.Cin;
    const double b_off = (ones_col && r == d.Cin) ? 1.0 : 0.0;
#pragma unroll 2
    for (int k = 0; k < PW_TILE / 16; ++k) {
      float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f), b4 = a4;
      if (a_on) a4 = *reinterpret_cast<const float4*>(sG + r * PW_LD + 16 * k + 4 * q);
      if (b_on) b4 = *reinterpret_cast<const float4*>(sX + r * PW_LD + 16 * k + 4 * q);
      const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        accM = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[j], b_on ? (double)bv[j] : b_off, accM, 0, 0, 0);
        if (!ones_col) accS = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[j], 1.0, accS, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // the four waves' tiles (D[(l >> 4) + 4 i][l & 15] in register i) and loss sums through LDS, added in wave order
  double* sD = reinterpret_cast<double*>(smem + PW_WF);            // [4][PW_ROW]: the staging area is free after the last barrier
  loss = wave_sum_d(loss);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = q + 4 * i;
    sD[wave * PW_ROW + co * PW_C + r] = accM[i];
    if (!ones_col && r == 0) sD[wave * PW_ROW + PW_C * PW_C + co] = accS[i];
  }
  if (lane == 0) sD[wave * PW_ROW + PW_C * PW_C + PW_C] = loss;
  __syncthreads();
  double* row = part + (size_t)blockIdx.x * PW_ROW;
  for (int e = threadIdx.x; e < PW_ROW; e += 256) {
    int src = e;
    if (ones_col && e >= PW_C * PW_C && e < PW_C * PW_C + PW_C) src = (e - PW_C * PW_C) * PW_C + d.Cin;      // s lives in column Cin of M
    double v = ((sD[src] + sD[PW_ROW + src]) + sD[2 * PW_ROW + src]) + sD[3 * PW_ROW + src];
    if (ones_col && e < PW_C * PW_C && (e & (PW_C - 1)) >= d.Cin) v = 0.0;
    row[e] = v;
  }
}

// One work-group: the partial rows summed in a fixed order in fp64 (four strided quarters, then the quarters in order), the small
// products in fp64, the flat fp32 gradient in parameter order and the fp64 loss sum.
__global__ __launch_bounds__(PW_FIN_THREADS) void k_pwreg_finalize(const double* __restrict__ part, int nblocks,
                                                                    const float* __restrict__ params, PwDims d, double scale,
                                                                    float* __restrict__ grad, double* __restrict__ loss_sum) {
  __shared__ double sQ[4][PW_ROW];
  __shared__ double sM[PW_C][PW_C];
  __shared__ double sS[PW_C];
  for (int w = threadIdx.x; w < 4 * PW_ROW; w += PW_FIN_THREADS) {
    const int e = w % PW_ROW, j = w / PW_ROW;
    double acc = 0.0;
#pragma unroll 8
    for (int b = j; b < nblocks; b += 4) acc += part[(size_t)b * PW_ROW + e];
    sQ[j][e] = acc;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < PW_ROW; e += PW_FIN_THREADS) {
    const double v = ((sQ[0][e] + sQ[1][e]) + sQ[2][e]) + sQ[3][e];
    if (e < PW_C * PW_C) sM[e / PW_C][e % PW_C] = v * scale;
    else if (e < PW_C * PW_C + PW_C) sS[e - PW_C * PW_C] = v * scale;
    else if (loss_sum) loss_sum[0] = v;
  }
  __syncthreads();
  const int n1 = d.C1 * d.Cin;
  if (d.layers == 1) {                       // dW = M, db = s
    for (int i = threadIdx.x; i < n1; i += PW_FIN_THREADS) grad[i] = (float)sM[i / d.Cin][i % d.Cin];
    for (int i = threadIdx.x; i < d.C1; i += PW_FIN_THREADS) grad[n1 + i] = (float)sS[i];
    return;
  }
  const float* W1 = params;
  const float* b1 = params + n1;
  const float* W2 = b1 + d.C1;
  const int n2 = d.Cout * d.C1;
  float* gW1 = grad;
  float* gb1 = grad + n1;
  float* gW2 = gb1 + d.C1;
  float* gb2 = gW2 + n2;
  for (int i = threadIdx.x; i < n1; i += PW_FIN_THREADS) {          // dW1 = W2^T M
    const int c1 = i / d.Cin, ci = i % d.Cin;
    double a = 0.0;
    for (int co = 0; co < d.Cout; ++co) a += (double)W2[co * d.C1 + c1] * sM[co][ci];
    gW1[i] = (float)a;
  }
  for (int c1 = threadIdx.x; c1 < d.C1; c1 += PW_FIN_THREADS) {     // db1 = W2^T s
    double a = 0.0;
    for (int co = 0; co < d.Cout; ++co) a += (double)W2[co * d.C1 + c1] * sS[co];
    gb1[c1] = (float)a;
  }
  for (int i = threadIdx.x; i < n2; i += PW_FIN_THREADS) {          // dW2 = M W1^T + s b1^T
    const int co = i / d.C1, c1 = i % d.C1;
    double a = sS[co] * (double)b1[c1];
    for (int ci = 0; ci < d.Cin; ++ci) a += sM[co][ci] * (double)W1[c1 * d.Cin + ci];
    gW2[i] = (float)a;
  }
  for (int co = threadIdx.x; co < d.Cout; co += PW_FIN_THREADS) gb2[co] = (float)sS[co];      // db2 = s
}

bool pw_dims_ok(int Cin, int C1, int Cout, int layers) {
  if (layers != 1 && layers != 2) return false;
  if (Cin < 1 || Cin > PW_C || C1 < 1 || C1 > PW_C || Cout < 1 || Cout > PW_C) return false;
  return layers == 2 || C1 == Cout;
}

bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

size_t sweep_smem_bytes(int Cin, int Cout) {
  const size_t stage = (size_t)4 * (Cin + Cout) * PW_LD * sizeof(float);
  const size_t fold = (size_t)4 * PW_ROW * sizeof(double);
  return PW_WF * sizeof(float) + (stage > fold ? stage : fold);
}

struct SweepArgs {
  const float* x; const float* yg; const float* params; PwDims d; size_t HW; int tpi; long long ntiles; int iters; double* part;
  int nb; size_t smem; hipStream_t st;
};

template <int MODE, bool VEC>
bool sweep_launch(const SweepArgs& a) {
  if (sc_lds_limit(&k_pwreg_sweep<MODE, VEC>, a.smem, "sc_pwreg_train_sweep") != SC_OK) return false;
  hipLaunchKernelGGL((k_pwreg_sweep<MODE, VEC>), dim3(a.nb), dim3(256), a.smem, a.st, a.x, a.yg, a.params, a.d, a.HW, a.tpi, a.ntiles,
                     a.iters, a.part);
  return true;
}

template <int MODE>
bool sweep_launch_mode(const SweepArgs& a, bool vec) { return vec ? sweep_launch<MODE, true>(a) : sweep_launch<MODE, false>(a); }

}  // namespace

extern "C" size_t sc_pwreg_param_floats(int Cin, int C1, int Cout, int layers) {
  if (!pw_dims_ok(Cin, C1, Cout, layers)) return 0;
  return (size_t)C1 * Cin + C1 + (layers == 2 ? (size_t)Cout * C1 + Cout : 0);
}

extern "C" int sc_pwreg_fwd(const float* x, const float* params, int N, int Cin, int C1, int Cout, int layers, int H, int W,
                            float* pred, sc_stream stream) {
  SC_REQUIRE(x && params && pred, "sc_pwreg_fwd: null pointer");
  SC_REQUIRE(pw_dims_ok(Cin, C1, Cout, layers), "sc_pwreg_fwd: channels must be 1..%d and layers 1 or 2 (got %d -> %d -> %d, %d layers)",
             PW_C, Cin, C1, Cout, layers);
  SC_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "sc_pwreg_fwd: bad shape N=%d H=%d W=%d", N, H, W);
  SC_REQUIRE(aligned_to(x, 4) && aligned_to(pred, 4) && aligned_to(params, 4), "sc_pwreg_fwd: misaligned pointer");
  const size_t HW = (size_t)H * W;
  const int vec = HW % 4 == 0 && aligned_to(x, 16) && aligned_to(pred, 16);
  const PwDims d = {Cin, C1, Cout, layers};
  const size_t gx = (HW + 1023) / 1024;
  SC_REQUIRE(gx <= 0x7fffffffu, "sc_pwreg_fwd: plane too large");
  if (vec) hipLaunchKernelGGL(k_pwreg_fwd<true>, dim3((unsigned)gx, N), dim3(256), 0, (hipStream_t)stream, x, params, d, HW, pred);
  else hipLaunchKernelGGL(k_pwreg_fwd<false>, dim3((unsigned)gx, N), dim3(256), 0, (hipStream_t)stream, x, params, d, HW, pred);
  SC_LAUNCH_OK("sc_pwreg_fwd");
  return SC_OK;
}

extern "C" int sc_reg_loss(const float* pred, const float* y, size_t n, int kind, double* loss_sum, float* dpred, double* work,
                           sc_stream stream) {
  SC_REQUIRE(pred && y && loss_sum && work && n > 0, "sc_reg_loss: bad argument");
  SC_REQUIRE(kind == SC_REG_L1 || kind == SC_REG_MSE, "sc_reg_loss: kind must be SC_REG_L1 or SC_REG_MSE, got %d", kind);
  const size_t want = (n + 1023) / 1024;
  const int nb = (int)(want < SC_REG_LOSS_PARTS ? want : SC_REG_LOSS_PARTS);
  const float inv_n = (float)(1.0 / (double)n);
  if (kind == SC_REG_L1)
    hipLaunchKernelGGL(k_reg_loss<SC_REG_L1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, pred, y, n, inv_n, dpred, work);
  else
    hipLaunchKernelGGL(k_reg_loss<SC_REG_MSE>, dim3(nb), dim3(256), 0, (hipStream_t)stream, pred, y, n, inv_n, dpred, work);
  SC_LAUNCH_OK("sc_reg_loss");
  hipLaunchKernelGGL(k_reg_loss_sum, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)work, nb, loss_sum);
  SC_LAUNCH_OK("sc_reg_loss (sum)");
  return SC_OK;
}

extern "C" int sc_pwreg_sweep_blocks(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  const size_t HW = (size_t)H * W;
  const size_t tiles = (size_t)N * ((HW + PW_TILE - 1) / PW_TILE);
  const size_t nb = (tiles + 3) / 4;
  return (int)(nb < PW_MAX_BLOCKS ? nb : PW_MAX_BLOCKS);
}

extern "C" int sc_pwreg_train_sweep(const float* x, const float* y_or_g, const float* params, int N, int Cin, int C1, int Cout,
                                    int layers, int H, int W, int mode, double* part, sc_stream stream) {
  SC_REQUIRE(x && y_or_g && part, "sc_pwreg_train_sweep: null pointer");
  SC_REQUIRE(mode == SC_REG_L1 || mode == SC_REG_MSE || mode == SC_PWREG_G_FROM_MEMORY, "sc_pwreg_train_sweep: bad mode %d", mode);
  SC_REQUIRE(params || mode == SC_PWREG_G_FROM_MEMORY, "sc_pwreg_train_sweep: null parameters");
  SC_REQUIRE(pw_dims_ok(Cin, C1, Cout, layers), "sc_pwreg_train_sweep: channels must be 1..%d and layers 1 or 2 (got %d -> %d -> %d, %d layers)",
             PW_C, Cin, C1, Cout, layers);
  SC_REQUIRE(N >= 1 && H >= 1 && W >= 1, "sc_pwreg_train_sweep: bad shape N=%d H=%d W=%d", N, H, W);
  SC_REQUIRE(aligned_to(x, 4) && aligned_to(y_or_g, 4) && aligned_to(part, 8), "sc_pwreg_train_sweep: misaligned pointer");
  const size_t HW = (size_t)H * W;
  const size_t tpi = (HW + PW_TILE - 1) / PW_TILE;
  SC_REQUIRE(tpi <= 0x7fffffffu, "sc_pwreg_train_sweep: plane too large");
  const long long ntiles = (long long)N * (long long)tpi;
  const int nb = sc_pwreg_sweep_blocks(N, H, W);
  const int iters = (int)((ntiles + (long long)nb * 4 - 1) / ((long long)nb * 4));
  const bool vec = HW % 2 == 0 && aligned_to(x, 8) && aligned_to(y_or_g, 8);
  const SweepArgs a = {x, y_or_g, params, {Cin, C1, Cout, layers}, HW, (int)tpi, ntiles, iters, part, nb, sweep_smem_bytes(Cin, Cout),
                       (hipStream_t)stream};
  bool ok;
  if (mode == SC_REG_L1) ok = sweep_launch_mode<SC_REG_L1>(a, vec);
  else if (mode == SC_REG_MSE) ok = sweep_launch_mode<SC_REG_MSE>(a, vec);
  else ok = sweep_launch_mode<SC_PWREG_G_FROM_MEMORY>(a, vec);
  SC_REQUIRE(ok, "sc_pwreg_train_sweep: cannot reserve %zu bytes of LDS", sweep_smem_bytes(PW_C, PW_C));
  SC_LAUNCH_OK("sc_pwreg_train_sweep");
  return SC_OK;
}

extern "C" int sc_pwreg_finalize(const double* part, int nblocks, const float* params, int Cin, int C1, int Cout, int layers,
                                 double scale, float* grad, double* loss_sum, sc_stream stream) {
  SC_REQUIRE(part && grad, "sc_pwreg_finalize: null pointer");
  SC_REQUIRE(pw_dims_ok(Cin, C1, Cout, layers), "sc_pwreg_finalize: channels must be 1..%d and layers 1 or 2 (got %d -> %d -> %d, %d layers)",
             PW_C, Cin, C1, Cout, layers);
  SC_REQUIRE(params || layers == 1, "sc_pwreg_finalize: a two-layer network needs its parameters");
  SC_REQUIRE(nblocks >= 1 && nblocks <= PW_MAX_BLOCKS, "sc_pwreg_finalize: nblocks %d outside 1..%d", nblocks, PW_MAX_BLOCKS);
  const PwDims d = {Cin, C1, Cout, layers};
  hipLaunchKernelGGL(k_pwreg_finalize, dim3(1), dim3(PW_FIN_THREADS), 0, (hipStream_t)stream, part, nblocks, params, d, scale, grad,
                     loss_sum);
  SC_LAUNCH_OK("sc_pwreg_finalize");
  return SC_OK;
}
