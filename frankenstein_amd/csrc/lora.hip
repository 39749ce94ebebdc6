// lora.hip — low-rank adapters (LoRA, Hu et al. 2021) on a frozen Linear:  y = x W^T + b + s (x A^T) B^T,  A [r, K], B [N, r], s = alpha / r.
// The base product stays with the GEMMs of gemm.hip; this file holds the three products that have one extent equal to r (4 .. 64), a
// shape none of the tiled GEMMs is built for, and the merge of the adapters into the weight.  Float64 restatement: tests/lora_ref.py.
//
// fk_lora_fwd: one launch,  u = round_to_dtype(x A^T)  and  out = (res or 0) + scale * colscale(n) * (u B^T).  A workgroup (4 waves) owns
//   32 rows.  First product, K split over the waves in k-steps of 16: the adapter row j is the A operand and the data row m the B
//   operand, so the 32 x 32 result X = u^T has the data row on the lane and j in its 16 registers (r <= 32: one such tile, r <= 64: two;
//   rows j >= r are zero operands).  The four partial tiles meet in LDS in the registers' own layout and every wave adds them in wave
//   order 0..3, so every wave then holds the whole X.  Rounded once to the compute dtype, those registers ARE the A operand of the second
//   product (fk_common.h: an accumulator tile as the next operand; it sums over X's row index j): Z[m][n] = sum_j X[j][m] B[n][j], the
//   column n on the lane, 32 columns per step.  B's fragment follows the permuted k order of that reuse, which comes in runs of four
//   consecutive j: that is why r % 4 == 0.  u never leaves the chip between the two products; wave 0 of the first column block stores it
//   for the backward.  Blocks along y take column ranges (each recomputes X: K * r * 32 MACs, x from L2), chosen from the shape alone.
//   The same entry point is the data gradient: x = dy, A = B^T [r, N], B = A^T [K, r], res = out = dh  gives  u = dy B  and  dh += s u A.
// fk_lora_wgrad: dB[n][j] (+)= s sum_m dy[m][n] u[m][j],  dA[j][k] (+)= s sum_m du[m][j] x[m][k]  with du the UNSCALED dy B that the
//   transposed fk_lora_fwd call stores (s du^T x = (s du)^T x).  Both are "wide column of the big operand times r small values": a lane
//   owns four columns of dy (or x) and 16 values of j, the small operand's row is the same for the whole wave.  Rows are split in slices
//   of 64; with more than one slice the partials go to the workspace in the layout of (dB, dA) and a second kernel adds them in slice
//   order: no atomics, the same bits on every run.  fp32 FMA on the vector unit: 2 M r (N + K) flops against M (N + K) elements read is
//   r / 2 MACs per byte at most, far below what the vector unit sustains per byte of HBM.
// fk_lora_merge: out[n][k] = fma(scale, chain, W[n][k]),  chain = fma(B[n][j], A[j][k], chain) for j = 0 .. r-1 from zero, all fp32; the
//   bf16 form stores the rounding of that same fp32 value.
#include "fk_common.h"

namespace {

constexpr int LF_TPB = 256;       // fk_lora_fwd: 4 waves
constexpr int LF_ROWS = 32;       // rows per workgroup
constexpr int LW_ROWS = 64;       // fk_lora_wgrad: rows per slice
constexpr int LW_COLS = 256;      // columns of dy / x per workgroup (one wave, four per lane)
constexpr int LW_J = 16;          // values of j per workgroup

// 8 elements at p of which the first `valid` exist (a multiple of 8 for bf16, of 4 for fp32, possibly <= 0); the rest are zero
template <typename T> FK_DEV void load8(Frag<T>& f, const T* p, int valid);
template <> FK_DEV void load8<bf16_t>(Frag<bf16_t>& f, const bf16_t* p, int valid) {
  frag_zero<bf16_t>(f);
  if (valid >= 8) f.v = *reinterpret_cast<const bf16x8*>(p);
}
template <> FK_DEV void load8<float>(Frag<float>& f, const float* p, int valid) {
  frag_zero<float>(f);
  if (valid >= 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) f.v[e] = a[e];
  }
  if (valid >= 8) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) f.v[4 + e] = b[e];
  }
}

// 4 elements at p (8-byte aligned for bf16, 16 for fp32) as fp32, and back
template <typename T> FK_DEV void load4(const T* p, float (&v)[4]);
template <> FK_DEV void load4<bf16_t>(const bf16_t* p, float (&v)[4]) {
  const bf16x4 a = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (float)a[e];
}
template <> FK_DEV void load4<float>(const float* p, float (&v)[4]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = a[e];
}
template <typename T> FK_DEV void store4(T* p, const float (&v)[4]);
template <> FK_DEV void store4<bf16_t>(bf16_t* p, const float (&v)[4]) {
  bf16x4 a;
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = (bf16_t)v[e];
  *reinterpret_cast<bf16x4*>(p) = a;
}
template <> FK_DEV void store4<float>(float* p, const float (&v)[4]) {
  f32x4 a;
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = v[e];
  *reinterpret_cast<f32x4*>(p) = a;
}

struct LoraFwdArgs {
  const void* x;
  const void* A;
  const void* B;
  const void* res;
  void* u_out;
  void* out;
  int64_t ldx, ldr, ldo;
  int M, N, K, r, q_cols, tiles_per_block;
  float scale, q_scale;
};

template <typename T, int JT>
__global__ __launch_bounds__(LF_TPB) void lora_fwd_kernel(LoraFwdArgs a) {
  __shared__ float red[4 * JT * 16 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
  const int M = a.M, N = a.N, K = a.K, r = a.r;
  const int m0 = blockIdx.x * LF_ROWS;
  const T* x = (const T*)a.x;
  const T* A = (const T*)a.A;
  const T* B = (const T*)a.B;

  // ---- X = A x^T over this wave's k-steps
  f32x16 X[JT];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int q = 0; q < 16; ++q) X[jt][q] = 0.0f;
  const bool mrow = m0 + i < M;
  const T* xrow = x + (mrow ? (int64_t)(m0 + i) * a.ldx : 0);
  const int nsteps = (K + 15) >> 4;
#pragma unroll 2
  for (int ks = wave; ks < nsteps; ks += 4) {
    const int kk = ks * 16 + 8 * h;
    Frag<T> fx;
    load8<T>(fx, xrow + kk, mrow ? K - kk : 0);
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      const int j = jt * 32 + i;
      Frag<T> fa;
      load8<T>(fa, A + (j < r ? (int64_t)j * K + kk : 0), j < r ? K - kk : 0);
      mma32<T>(X[jt], fa, fx);
    }
  }
  // ---- the four partial tiles, added in wave order by every wave
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int q = 0; q < 16; ++q) red[((wave * JT + jt) * 16 + q) * 64 + lane] = X[jt][q];
  __syncthreads();
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float* p = red + (jt * 16 + q) * 64 + lane;
      X[jt][q] = ((p[0] + p[JT * 16 * 64]) + p[2 * JT * 16 * 64]) + p[3 * JT * 16 * 64];
    }
  // ---- u: one rounding to the compute dtype; the operand of the second product and the tensor the backward reads
  Frag<T> fu[JT][2];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int s = 0; s < 2; ++s) frag_from_acc<T>(fu[jt][s], X[jt], s);
  if (a.u_out && blockIdx.y == 0 && wave == 0 && mrow) {
    T* u = (T*)a.u_out + (int64_t)(m0 + i) * r;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {            // registers 4q .. 4q+3 are the consecutive rows 8q + 4h .. + 3 of the tile
        const int j = jt * 32 + 8 * q + 4 * h;
        if (j < r) {
          const float v[4] = {X[jt][4 * q], X[jt][4 * q + 1], X[jt][4 * q + 2], X[jt][4 * q + 3]};
          store4<T>(u + j, v);
        }
      }
  }
  // ---- Z = X^T B^T, 32 columns at a time
  const int ntile = (N + 31) >> 5;
  const T* res = (const T*)a.res;
  T* out = (T*)a.out;
  for (int it = wave; it < a.tiles_per_block; it += 4) {
    const int t = blockIdx.y * a.tiles_per_block + it;
    if (t >= ntile) break;
    const int n = t * 32 + i;
    const bool ncol = n < N;
    f32x16 Z;
#pragma unroll
    for (int q = 0; q < 16; ++q) Z[q] = 0.0f;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (jt * 32 + 16 * s < r) {            // uniform
          // k-slot (h, e) of this step is row jt * 32 + acc_row_of_slot(s, h, e) of X: two runs of four consecutive j
          const int ja = jt * 32 + 16 * s + 4 * h, jb = ja + 8;
          float va[4] = {0.0f, 0.0f, 0.0f, 0.0f}, vb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if (ncol && ja < r) load4<T>(B + (int64_t)n * r + ja, va);
          if (ncol && jb < r) load4<T>(B + (int64_t)n * r + jb, vb);
          Frag<T> fb;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            frag_set<T>(fb, e, va[e]);
            frag_set<T>(fb, 4 + e, vb[e]);
          }
          mma32<T>(Z, fu[jt][s], fb);
        }
      }
    if (ncol) {
      const float cs = a.scale * (n < a.q_cols ? a.q_scale : 1.0f);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = m0 + acc_row(q, h);
        if (m < M) {
          const float base = res ? to_f32<T>(res[(int64_t)m * a.ldr + n]) : 0.0f;
          out[(int64_t)m * a.ldo + n] = from_f32<T>(fmaf(cs, Z[q], base));
        }
      }
    }
  }
}

struct LoraWgArgs {
  const void* dy;
  const void* u;
  const void* du;
  const void* x;
  float* dA;
  float* dB;
  float* ws;
  int M, N, K, r, S, nbN, accumulate;
  float scale;
};

// the (dB, dA) image: dB [N][r] first, dA [r][K] behind it
FK_DEV void lora_wg_final(float* dst, const float (&v)[4], float scale, int accumulate) {
  float o[4];
  if (accumulate) load4<float>(dst, o);
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = accumulate ? fmaf(scale, v[e], o[e]) : scale * v[e];
  store4<float>(dst, o);
}

template <typename T>
__global__ __launch_bounds__(64) void lora_wgrad_kernel(LoraWgArgs a) {
  const int lane = threadIdx.x, r = a.r, N = a.N, K = a.K;
  const bool isB = (int)blockIdx.x < a.nbN;
  const T* big = (const T*)(isB ? a.dy : a.x);
  const T* small = (const T*)(isB ? a.u : a.du);
  const int ncols = isB ? N : K;
  const int c = (isB ? blockIdx.x : blockIdx.x - a.nbN) * LW_COLS + lane * 4;
  const int s = blockIdx.y, j0 = blockIdx.z * LW_J;
  const int nj = r - j0 < LW_J ? r - j0 : LW_J;                  // a multiple of 4
  const int m_lo = s * LW_ROWS, m_hi = m_lo + LW_ROWS < a.M ? m_lo + LW_ROWS : a.M;
  const bool cv = c < ncols;                                      // ncols % 4 == 0: all four columns or none
  float acc[4][LW_J];
#pragma unroll
  for (int cc = 0; cc < 4; ++cc)
#pragma unroll
    for (int jj = 0; jj < LW_J; ++jj) acc[cc][jj] = 0.0f;
#pragma unroll 4
  for (int m = m_lo; m < m_hi; ++m) {
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (cv) load4<T>(big + (int64_t)m * ncols + c, v);
#pragma unroll
    for (int g = 0; g < LW_J / 4; ++g) {
      if (4 * g < nj) {                                           // uniform
        float sv[4];
        load4<T>(small + (int64_t)m * r + j0 + 4 * g, sv);        // one address for the whole wave
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[cc][4 * g + e] = fmaf(v[cc], sv[e], acc[cc][4 * g + e]);
      }
    }
  }
  if (!cv) return;
  const int64_t total = (int64_t)N * r + (int64_t)r * K;
  const bool fin = a.S == 1;
  float* img_B = fin ? a.dB : a.ws + (int64_t)s * total;
  float* img_A = fin ? a.dA : a.ws + (int64_t)s * total + (int64_t)N * r;
  if (isB) {
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
#pragma unroll
      for (int g = 0; g < LW_J / 4; ++g) {
        if (4 * g < nj) {
          const float v[4] = {acc[cc][4 * g], acc[cc][4 * g + 1], acc[cc][4 * g + 2], acc[cc][4 * g + 3]};
          float* dst = img_B + (int64_t)(c + cc) * r + j0 + 4 * g;
          if (fin) lora_wg_final(dst, v, a.scale, a.accumulate);
          else store4<float>(dst, v);
        }
      }
  } else {
#pragma unroll
    for (int jj = 0; jj < LW_J; ++jj) {
      if (jj < nj) {
        const float v[4] = {acc[0][jj], acc[1][jj], acc[2][jj], acc[3][jj]};
        float* dst = img_A + (int64_t)(j0 + jj) * K + c;
        if (fin) lora_wg_final(dst, v, a.scale, a.accumulate);
        else store4<float>(dst, v);
      }
    }
  }
}

// four elements of the (dB, dA) image per thread: the slices' partials in slice order
__global__ __launch_bounds__(FK_TPB) void lora_wgrad_reduce_kernel(LoraWgArgs a) {
  const int64_t nB = (int64_t)a.N * a.r, total = nB + (int64_t)a.r * a.K;
  const int64_t e = ((int64_t)blockIdx.x * FK_TPB + threadIdx.x) * 4;
  if (e >= total) return;
  float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int s = 0; s < a.S; ++s) {
    float p[4];
    load4<float>(a.ws + (int64_t)s * total + e, p);
#pragma unroll
    for (int q = 0; q < 4; ++q) sum[q] += p[q];
  }
  lora_wg_final(e < nB ? a.dB + e : a.dA + (e - nB), sum, a.scale, a.accumulate);
}

struct LoraMergeArgs {
  const float* W;
  const float* A;
  const float* B;
  void* out;
  int64_t ldo;
  int N, K, r;
  float scale;
};

template <typename T>
__global__ __launch_bounds__(FK_TPB) void lora_merge_kernel(LoraMergeArgs a) {
  const int kg = a.K >> 2;
  const int64_t idx = (int64_t)blockIdx.x * FK_TPB + threadIdx.x;
  if (idx >= (int64_t)a.N * kg) return;
  const int n = (int)(idx / kg), k = (int)(idx - (int64_t)n * kg) * 4;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int j = 0; j < a.r; ++j) {
    const float b = a.B[(int64_t)n * a.r + j];
    float av[4];
    load4<float>(a.A + (int64_t)j * a.K + k, av);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaf(b, av[e], acc[e]);
  }
  float w[4];
  load4<float>(a.W + (int64_t)n * a.K + k, w);
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = fmaf(a.scale, acc[e], w[e]);
  store4<T>((T*)a.out + (int64_t)n * a.ldo + k, w);
}

int lora_check(const char* name, int64_t M, int64_t N, int64_t K, int64_t r, int dtype) {
  if (fk_lora_route(M, N, K, r, dtype) < 0)
    return fk_set_error(FK_EINVAL,
                        "%s: outside the envelope (M %lld, N %lld, K %lld, r %lld, dtype %d: bf16 or fp32, 4 <= r <= 64 with r %% 4 == 0, N and K "
                        "multiples of 8 (4 for fp32), M >= 1, all below 2^31)",
                        name, (long long)M, (long long)N, (long long)K, (long long)r, dtype);
  return FK_OK;
}

bool lora_aligned(const void* p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

}  // namespace

extern "C" {

int fk_lora_route(int64_t M, int64_t N, int64_t K, int64_t r, int dtype) {
  if (dtype != FK_F32 && dtype != FK_BF16) return -1;
  const int64_t lim = 1LL << 31, g = dtype == FK_BF16 ? 8 : 4;
  if (M < 1 || N < 1 || K < 1 || M >= lim || N >= lim || K >= lim) return -1;
  if (r < 4 || r > 64 || r % 4 != 0 || N % g != 0 || K % g != 0) return -1;
  return r <= 32 ? FK_LORA_R32 : FK_LORA_R64;
}

int fk_lora_fwd(const void* x, int64_t ldx, const void* A, const void* B, int64_t M, int64_t N, int64_t K, int64_t r, float scale,
                int64_t q_cols, float q_scale, const void* res, int64_t ldr, void* u_out, void* out, int64_t ldo, int dtype, void* stream) {
  if (int rc = lora_check("fk_lora_fwd", M, N, K, r, dtype)) return rc;
  FK_CHECK_ARG(x && A && B && out, "fk_lora_fwd: null pointer");
  const int64_t lim = 1LL << 31, g = dtype == FK_BF16 ? 8 : 4;
  FK_CHECK_ARG(ldx >= K && ldo >= N && (!res || ldr >= N) && ldx < lim && ldo < lim && ldr < lim, "fk_lora_fwd: leading dimensions must cover their rows and stay below 2^31");
  FK_CHECK_ARG(ldx % g == 0, "fk_lora_fwd: ldx must be a multiple of 16 bytes");
  FK_CHECK_ARG(q_cols >= 0 && q_cols <= N, "fk_lora_fwd: q_cols = %lld outside [0, N]", (long long)q_cols);
  const size_t el = dtype == FK_BF16 ? 2 : 4;
  FK_CHECK_ARG(lora_aligned(x, 16) && lora_aligned(A, 16) && lora_aligned(B, 4 * el) && lora_aligned(u_out, 4 * el) && lora_aligned(out, el) &&
                   lora_aligned(res, el),
               "fk_lora_fwd: misaligned pointer");
  const int64_t mt = fk_cdiv(M, LF_ROWS), ntile = fk_cdiv(N, 32);
  // column ranges along y: about two workgroups per CU, at least one tile per wave
  int64_t by = fk_cdiv(512, mt);
  if (by > fk_cdiv(ntile, 4)) by = fk_cdiv(ntile, 4);
  if (by < 1) by = 1;
  const int64_t tpb = fk_cdiv(ntile, by);
  by = fk_cdiv(ntile, tpb);
  const LoraFwdArgs a{x, A, B, res, u_out, out, ldx, ldr, ldo, (int)M, (int)N, (int)K, (int)r, (int)q_cols, (int)tpb, scale, q_scale};
  const dim3 grid((unsigned)mt, (unsigned)by);
  hipStream_t s = (hipStream_t)stream;
  if (r <= 32) FK_BY_DTYPE(dtype, T, hipLaunchKernelGGL((lora_fwd_kernel<T, 1>), grid, dim3(LF_TPB), 0, s, a));
  else FK_BY_DTYPE(dtype, T, hipLaunchKernelGGL((lora_fwd_kernel<T, 2>), grid, dim3(LF_TPB), 0, s, a));
  FK_CHECK_LAUNCH("fk_lora_fwd");
  return FK_OK;
}

size_t fk_lora_wgrad_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t r) {
  if (M < 1 || N < 1 || K < 1 || r < 1) return 0;
  const int64_t S = fk_cdiv(M, LW_ROWS);
  return S > 1 ? (size_t)S * (size_t)(N * r + r * K) * sizeof(float) : 0;
}

int fk_lora_wgrad(const void* dy, const void* u, const void* du, const void* x, int64_t M, int64_t N, int64_t K, int64_t r, float scale,
                  float* dA, float* dB, int accumulate, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = lora_check("fk_lora_wgrad", M, N, K, r, dtype)) return rc;
  FK_CHECK_ARG(dy && u && du && x && dA && dB, "fk_lora_wgrad: null pointer");
  const size_t el = dtype == FK_BF16 ? 2 : 4;
  FK_CHECK_ARG(lora_aligned(dy, 4 * el) && lora_aligned(x, 4 * el) && lora_aligned(u, 4 * el) && lora_aligned(du, 4 * el) && lora_aligned(dA, 16) &&
                   lora_aligned(dB, 16) && lora_aligned(workspace, 16),
               "fk_lora_wgrad: misaligned pointer");
  const int64_t S = fk_cdiv(M, LW_ROWS), total = N * r + r * K;
  FK_CHECK_ARG(S <= 65535, "fk_lora_wgrad: M = %lld needs more than 65535 row slices", (long long)M);
  FK_CHECK_ARG(S == 1 || (workspace && workspace_bytes >= fk_lora_wgrad_workspace_bytes(M, N, K, r)), "fk_lora_wgrad: workspace too small");
  const int64_t nbN = fk_cdiv(N, LW_COLS), nbK = fk_cdiv(K, LW_COLS);
  const LoraWgArgs a{dy, u, du, x, dA, dB, (float*)workspace, (int)M, (int)N, (int)K, (int)r, (int)S, (int)nbN, accumulate, scale};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(nbN + nbK), (unsigned)S, (unsigned)fk_cdiv(r, LW_J));
  FK_BY_DTYPE(dtype, T, hipLaunchKernelGGL(lora_wgrad_kernel<T>, grid, dim3(64), 0, s, a));
  FK_CHECK_LAUNCH("fk_lora_wgrad(partials)");
  if (S > 1) {
    hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)fk_cdiv(total / 4, FK_TPB)), dim3(FK_TPB), 0, s, a);
    FK_CHECK_LAUNCH("fk_lora_wgrad");
  }
  return FK_OK;
}

int fk_lora_merge(const float* W, const float* A, const float* B, int64_t N, int64_t K, int64_t r, float scale, void* out, int64_t ldo,
                  int out_dtype, void* stream) {
  if (int rc = lora_check("fk_lora_merge", 1, N, K, r, out_dtype)) return rc;
  FK_CHECK_ARG(W && A && B && out, "fk_lora_merge: null pointer");
  FK_CHECK_ARG(ldo >= K && ldo < (1LL << 31) && ldo % 4 == 0, "fk_lora_merge: ldo must cover a row, stay below 2^31 and be a multiple of 4");
  FK_CHECK_ARG(lora_aligned(W, 16) && lora_aligned(A, 16) && lora_aligned(B, 4) && lora_aligned(out, out_dtype == FK_BF16 ? 8 : 16),
               "fk_lora_merge: misaligned pointer");
  const LoraMergeArgs a{W, A, B, out, ldo, (int)N, (int)K, (int)r, scale};
  const int64_t blocks = fk_cdiv(N * (K / 4), FK_TPB);
  FK_CHECK_ARG(blocks < (1LL << 31), "fk_lora_merge: N * K too large");
  hipStream_t s = (hipStream_t)stream;
  FK_BY_DTYPE(out_dtype, T, hipLaunchKernelGGL(lora_merge_kernel<T>, dim3((unsigned)blocks), dim3(FK_TPB), 0, s, a));
  FK_CHECK_LAUNCH("fk_lora_merge");
  return FK_OK;
}

}  // extern "C"
