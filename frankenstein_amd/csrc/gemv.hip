// gemv.hip — weight-streaming skinny GEMM for the single-token decode step (1 <= M <= 16 rows against a [N, K] weight):
//   fk_gemv_nt   C[m, n] = act( sum_k LN?(A[m, :])[k] * W[n, k] + bias[n] ) + residual[m, n]
// the nn.Linear call sites of the cached GPT decode step (models/gpt2_model.py:35,37,56,75,82-90,133 at t = 1), with the LayerNorm in
// front of c_attn / c_fc / lm_head (:27) and the exact-erf GELU behind c_fc (:83,89) folded into the launch.
//
// The MFMA GEMM cuts N into 128-row tiles: at d = 768 that is 6-24 workgroups on a 256-CU chip, each issuing 128 rows of matrix work
// for 1-5 real ones.  Here the product is what it is at this size, a stream of the weight matrix:
//   * a wave owns CW consecutive output columns (weight rows); its 64 lanes split K in 16-byte pieces, piece p -> lane p % 64;
//   * weights go global -> VGPR with the non-temporal hint (each byte is read once per launch), gv_unroll(CW) * CW loads in flight per lane
//     before the first one is consumed, no LDS round trip;
//   * the M activation rows are staged once per workgroup in LDS as fp32 (after the LayerNorm, whose statistics each workgroup
//     recomputes for its M rows: M * K elements out of L2, one load per element when the row fits the LDS chunk), bf16 pieces split
//     into two planes so that every ds_read_b128 is lane-linear; the first weight batch is already in flight while this happens;
//   * fp32 accumulators per (row, column); across lanes a fixed xor butterfly 32, 16, .., 1 in its reduce-scatter form (a lane keeps
//     half of its values at every step), which leaves value (m, c) in one lane that then runs the epilogue for it.
// No split-K over workgroups, no atomics, no workspace: deterministic and graph-capturable.
// Batch invariance: the lane <-> k mapping (piece g -> lane g % 64: every LDS chunk is a whole number of lane rounds), the per-lane order
// (pieces ascending, explicit fmaf per element) and the butterfly do not depend on the row bucket MB, on CW or on the LDS chunk length, so row m of an M = 16 call has the bits of the M = 1 call on that row.
#include "fk_common.h"

namespace {

constexpr int GV_WAVES = 4;          // waves per workgroup
// 16-byte weight pieces per column a lane has in flight: 8 loads per lane at two and four columns, 4 at one
constexpr int gv_unroll(int CW) { return CW >= 4 ? 2 : 4; }
// fp32 elements of one activation row that LDS holds at a time (longer rows are walked in chunks of this length).  A chunk is a whole
// number of 64-piece lane rounds in both dtypes (static_assert in the kernel), so piece g of a row sits in lane g % 64 whatever the chunk.
constexpr int gv_chunk(int MB) { return MB >= 16 ? 1024 : MB >= 8 ? 1536 : 3072; }
constexpr int GV_LDS_MAX = 16 * gv_chunk(16) * 4;
static_assert(GV_LDS_MAX <= 64 * 1024, "fk_gemv_nt: static LDS, two workgroups per CU at sixteen rows");
static_assert(8 * gv_chunk(8) * 4 <= GV_LDS_MAX && 4 * gv_chunk(4) * 4 <= GV_LDS_MAX, "fk_gemv_nt: LDS budget");

struct GemvArgs {
  const void* A; const void* W; void* C; const void* bias; const void* res;
  const float* gamma; const float* beta;
  int64_t lda, ldw, ldc, ldr;
  int M, N, K;
  float eps;
  int gelu, out_f32;
};

// element e of a 16-byte weight piece held as four dwords
template <typename T> FK_DEV float gv_welem(const u32x4& w, int e);
template <> FK_DEV float gv_welem<bf16_t>(const u32x4& w, int e) {
  const unsigned d = w[e >> 1];
  return __uint_as_float((e & 1) ? (d & 0xffff0000u) : (d << 16));
}
template <> FK_DEV float gv_welem<float>(const u32x4& w, int e) { return __uint_as_float(w[e]); }

// sum over the wave of NV values per lane (NV a power of two <= 64): butterfly 32, 16, .., 1.  While more than one value is left a
// lane keeps one half of them (the upper half where its lane bit is set) and adds its partner's copy of that half; the sums are the
// ones the plain `v += shfl_xor(v, o)` tree gives, bit for bit.  Returns the total of value gv_owned(lane).
template <int N, int O> FK_DEV void gv_reduce_step(float* v, int lane) {
  if constexpr (O > 0) {
    if constexpr (N > 1) {
      const bool up = (lane & O) != 0;
#pragma unroll
      for (int i = 0; i < N / 2; ++i) {
        const float keep = up ? v[i + N / 2] : v[i], send = up ? v[i] : v[i + N / 2];
        v[i] = keep + __shfl_xor(send, O, 64);
      }
      gv_reduce_step<N / 2, O / 2>(v, lane);
    } else {
      v[0] += __shfl_xor(v[0], O, 64);
      gv_reduce_step<1, O / 2>(v, lane);
    }
  }
}
template <int NV> FK_DEV float gv_reduce(float (&v)[NV], int lane) {
  static_assert(NV >= 1 && NV <= 64 && (NV & (NV - 1)) == 0, "power of two");
  gv_reduce_step<NV, 32>(v, lane);
  return v[0];
}
template <int N, int O> FK_DEV int gv_owned_step(int lane) {
  if constexpr (O > 0 && N > 1) return ((lane & O) ? N / 2 : 0) + gv_owned_step<N / 2, O / 2>(lane);
  else return 0;
}
template <int NV> FK_DEV int gv_owned(int lane) { return gv_owned_step<NV, 32>(lane); }

template <typename T, int MB, int CW>
__global__ __launch_bounds__(GV_WAVES * 64) void gemv_nt_kernel(const GemvArgs a) {
  constexpr int E = VecIO<T>::N;            // elements per 16-byte piece
  constexpr int F = gv_chunk(MB);           // fp32 elements of a row in LDS
  constexpr int FP = F / E;                 // = pieces of a chunk
  constexpr int PLANE = F / (E / 4);        // bf16: elements 0-3 of every piece in plane 0, 4-7 in plane 1
  constexpr int NV = MB * CW;
  constexpr int GV_U = gv_unroll(CW);
  constexpr int RPW = (MB + GV_WAVES - 1) / GV_WAVES;   // rows a wave stages (rows wave, wave + 4, ..)
  constexpr int SPL = FP / 64;              // pieces of a chunk a lane stages per row
  static_assert(FP % 64 == 0, "piece g of a row must sit in lane g % 64 in every row bucket (batch invariance)");
  __shared__ __attribute__((aligned(16))) float sx[MB * F];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* A = (const T*)a.A;
  const T* W = (const T*)a.W;
  const int M = a.M, N = a.N, K = a.K;
  const int np = K / E;

  // this wave's weight rows (clamped: a column past N is computed from row N - 1 and not stored)
  const int c0 = (blockIdx.x * GV_WAVES + wave) * CW;
  const T* wrow[CW];
#pragma unroll
  for (int c = 0; c < CW; ++c) wrow[c] = W + (int64_t)min(c0 + c, N - 1) * a.ldw;

  // one batch of weight pieces: GV_U per column, every load issued before the first is consumed; a lane past the end of the chunk
  // re-reads piece 0 and drops it in consume().  The first batch is issued before anything else, so that its trip to HBM runs beside
  // the LayerNorm and the staging of the activations; every later one right after the batch before it has been consumed.
  u32x4 w[CW][GV_U];
  auto issue = [&](int p0, int npc, int j0) {
#pragma unroll
    for (int u = 0; u < GV_U; ++u) {
      if (j0 + 64 * u < npc) {              // wave-uniform
        const int p = j0 + 64 * u + lane;
        const int64_t off = (int64_t)(p0 + (p < npc ? p : 0)) * E;
#pragma unroll
        for (int c = 0; c < CW; ++c) w[c][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[c] + off));
      }
    }
  };
  int p0 = 0, j0 = 0, npc = min(FP, np);
  issue(p0, npc, j0);

  // LayerNorm over a row longer than one LDS chunk: statistics in two passes over global memory first (like fk_norm_fwd).  A row
  // that fits one chunk (every LayerNorm of the decode step) gets them from the registers it is staged through, below.
  const bool ln = a.gamma != nullptr, ln_staged = ln && np <= FP;
  float mu[RPW], rs[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) { mu[r] = 0.0f; rs[r] = 1.0f; }
  if (ln && !ln_staged) {
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int m = wave + r * GV_WAVES;
      if (m < M) {
        const T* xr = A + (int64_t)m * a.lda;
        float v[E], s = 0.0f, q = 0.0f;
        for (int p = lane; p < np; p += 64) {
          VecIO<T>::load(xr + p * E, v);
#pragma unroll
          for (int e = 0; e < E; ++e) s += v[e];
        }
        const float mean = wave_sum(s) / K;
        for (int p = lane; p < np; p += 64) {
          VecIO<T>::load(xr + p * E, v);
#pragma unroll
          for (int e = 0; e < E; ++e) q = __builtin_fmaf(v[e] - mean, v[e] - mean, q);
        }
        mu[r] = mean;
        rs[r] = rsqrtf(wave_sum(q) / K + a.eps);
      }
    }
  }

  float acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.0f;

  while (true) {
    if (j0 == 0) {
      // stage chunk [p0, p0 + npc) of this wave's rows: every load first (clamped addresses, no branches around them), then
      // statistics / normalisation / LDS writes row by row
      if (p0) __syncthreads();
      u32x4 raw[RPW][SPL];
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const T* xr = A + (int64_t)min(wave + r * GV_WAVES, M - 1) * a.lda + (int64_t)p0 * E;
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
          const int p = lane + 64 * s;
          if (64 * s < npc) raw[r][s] = *reinterpret_cast<const u32x4*>(xr + (p < npc ? p : 0) * E);   // wave-uniform guard
        }
      }
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const int m = wave + r * GV_WAVES;
        if (m < M) {                        // wave-uniform
          if (ln_staged) {
            float s1 = 0.0f, q = 0.0f;
#pragma unroll
            for (int s = 0; s < SPL; ++s)
              if (lane + 64 * s < npc) {
#pragma unroll
                for (int e = 0; e < E; ++e) s1 += gv_welem<T>(raw[r][s], e);
              }
            const float mean = wave_sum(s1) / K;
#pragma unroll
            for (int s = 0; s < SPL; ++s)
              if (lane + 64 * s < npc) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                  const float d = gv_welem<T>(raw[r][s], e) - mean;
                  q = __builtin_fmaf(d, d, q);
                }
              }
            mu[r] = mean;
            rs[r] = rsqrtf(wave_sum(q) / K + a.eps);
          }
#pragma unroll
          for (int s = 0; s < SPL; ++s) {
            const int p = lane + 64 * s;
            if (p < npc) {
              float v[E];
#pragma unroll
              for (int e = 0; e < E; ++e) v[e] = gv_welem<T>(raw[r][s], e);
              if (ln) {
                const float* g = a.gamma + (int64_t)(p0 + p) * E;
#pragma unroll
                for (int e = 0; e < E; ++e) v[e] = (v[e] - mu[r]) * rs[r];
                if (a.beta) {
                  const float* b = a.beta + (int64_t)(p0 + p) * E;
#pragma unroll
                  for (int e = 0; e < E; ++e) v[e] = __builtin_fmaf(v[e], g[e], b[e]);
                } else {
#pragma unroll
                  for (int e = 0; e < E; ++e) v[e] *= g[e];
                }
              }
#pragma unroll
              for (int h = 0; h < E / 4; ++h) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = v[4 * h + e];
                *reinterpret_cast<f32x4*>(&sx[m * F + h * PLANE + p * 4]) = o;
              }
            }
          }
        }
      }
      __syncthreads();
    }

    // consume the batch in flight
#pragma unroll
    for (int u = 0; u < GV_U; ++u) {
      if (j0 + 64 * u < npc) {
        const int p = j0 + 64 * u + lane;
        const bool ok = p < npc;
        const int pl = ok ? p : 0;
        if (!ok) {
#pragma unroll
          for (int c = 0; c < CW; ++c) w[c][u] = u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          if (m < M) {                      // wave-uniform: skips the bucket's unused rows
            float x[E];
#pragma unroll
            for (int h = 0; h < E / 4; ++h) {
              const f32x4 t = *reinterpret_cast<const f32x4*>(&sx[m * F + h * PLANE + pl * 4]);
#pragma unroll
              for (int e = 0; e < 4; ++e) x[4 * h + e] = t[e];
            }
#pragma unroll
            for (int c = 0; c < CW; ++c) {
#pragma unroll
              for (int e = 0; e < E; ++e) acc[m * CW + c] = __builtin_fmaf(x[e], gv_welem<T>(w[c][u], e), acc[m * CW + c]);
            }
          }
        }
      }
    }

    j0 += 64 * GV_U;
    if (j0 >= npc) {
      p0 += FP;
      if (p0 >= np) break;
      npc = min(FP, np - p0);
      j0 = 0;
    }
    issue(p0, npc, j0);
  }

  const float total = gv_reduce<NV>(acc, lane);
  if ((lane & (64 / NV - 1)) != 0) return;
  const int idx = gv_owned<NV>(lane);
  const int m = idx / CW, col = c0 + idx % CW;
  if (m >= M || col >= N) return;
  float y = total;
  if (a.bias) y += to_f32<T>(((const T*)a.bias)[col]);
  if (a.gelu) y = fk_gelu(y);
  if (a.res) y += to_f32<T>(((const T*)a.res)[(int64_t)m * a.ldr + col]);
  if (a.out_f32) ((float*)a.C)[(int64_t)m * a.ldc + col] = y;
  else ((T*)a.C)[(int64_t)m * a.ldc + col] = from_f32<T>(y);
}

template <typename T, int MB> void gv_launch_cw(const GemvArgs& a, int cw, hipStream_t s) {
  const unsigned grid = (unsigned)fk_cdiv(fk_cdiv(a.N, cw), GV_WAVES);
  if (cw == 4) hipLaunchKernelGGL((gemv_nt_kernel<T, MB, 4>), dim3(grid), dim3(GV_WAVES * 64), 0, s, a);
  else if (cw == 2) hipLaunchKernelGGL((gemv_nt_kernel<T, MB, 2>), dim3(grid), dim3(GV_WAVES * 64), 0, s, a);
  else hipLaunchKernelGGL((gemv_nt_kernel<T, MB, 1>), dim3(grid), dim3(GV_WAVES * 64), 0, s, a);
}

template <typename T> void gv_launch(const GemvArgs& a, hipStream_t s) {
  // columns per wave: as many as still leave 1024 waves (four per CU); at 16 rows at least two, so that the LDS reads of the
  // activations (M * 32 bytes per 16-byte weight piece in bf16) stay below what the weight stream needs
  int cw = a.N >= 4 * 1024 ? 4 : a.N >= 2 * 1024 ? 2 : 1;
  if (a.M > 8 && cw < 2) cw = 2;
  if (a.M > 8) gv_launch_cw<T, 16>(a, cw, s);
  else if (a.M > 4) gv_launch_cw<T, 8>(a, cw, s);
  else if (a.M > 2) gv_launch_cw<T, 4>(a, cw, s);
  else if (a.M > 1) gv_launch_cw<T, 2>(a, cw, s);
  else gv_launch_cw<T, 1>(a, cw, s);
}

}  // namespace

extern "C" int fk_gemv_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                          const void* bias, const void* residual, int64_t ldr, const float* ln_gamma, const float* ln_beta, float ln_eps,
                          int flags, int dtype, int out_dtype, void* stream) {
  FK_DT_CHECK("fk_gemv_nt");
  FK_CHECK_ARG(out_dtype == dtype || out_dtype == FK_F32, "fk_gemv_nt: out_dtype must be dtype or FK_F32");
  FK_CHECK_ARG(M >= 1 && M <= 16, "fk_gemv_nt: M = %lld outside 1..16 (larger products belong to fk_gemm_nt)", (long long)M);
  const int64_t esz = dtype == FK_BF16 ? 2 : 4, vec = 16 / esz, lim = INT32_MAX;
  FK_CHECK_ARG(N > 0 && K > 0 && N <= lim && K <= lim, "fk_gemv_nt: empty problem or N / K beyond int32");
  FK_CHECK_ARG(K % vec == 0, "fk_gemv_nt: K must be a multiple of %lld (16 bytes)", (long long)vec);
  FK_CHECK_ARG(A && W && C, "fk_gemv_nt: null pointer");
  FK_CHECK_ARG(lda >= K && ldw >= K && ldc >= N && (!residual || ldr >= N), "fk_gemv_nt: leading dimensions must cover their rows");
  FK_CHECK_ARG(lda <= lim && ldw <= lim && ldc <= lim && ldr <= lim, "fk_gemv_nt: leading dimension beyond int32");
  FK_CHECK_ARG(((uintptr_t)A | (uintptr_t)W) % 16 == 0 && (M == 1 || lda % vec == 0) && (N == 1 || ldw % vec == 0),
               "fk_gemv_nt: A and W rows must be 16-byte aligned");
  FK_CHECK_ARG((flags & ~FK_GEMV_GELU) == 0, "fk_gemv_nt: unknown flags %d", flags);
  FK_CHECK_ARG(ln_gamma || !ln_beta, "fk_gemv_nt: ln_beta without ln_gamma");
  GemvArgs a{A, W, C, bias, residual, ln_gamma, ln_beta, lda, ldw, ldc, ldr, (int)M, (int)N, (int)K, ln_eps,
             (flags & FK_GEMV_GELU) ? 1 : 0, (out_dtype == FK_F32 && dtype != FK_F32) ? 1 : 0};
  FK_BY_DTYPE(dtype, T, gv_launch<T>(a, (hipStream_t)stream));
  FK_CHECK_LAUNCH("fk_gemv_nt");
  return FK_OK;
}
