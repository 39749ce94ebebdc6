// dayadapt.hip — the per-session input adapter in front of the patch tokeniser.  date_info[b] names the recording session ("day") of
// sample b; electrode drift between days is taken out by a small day-specific linear layer on the raw channels.  The rule (build-defined:
// the reference plumbs date_info through and never reads it; restated in float64 in tests/day_adapter_ref.py), with C = n_electrodes:
//
//     d = day[b]                                                       int64 on the device, never read by the host
//     y[b, t, :] = x[b, t, :] + x[b, t, :] @ delta[d] + bias[d]        0 <= d < n_days
//     y[b, t, :] = x[b, t, :]                                          any other d (-1 = unknown session), or day == NULL
//     tok[b, (t / P) * C + c, p] = round_to_dtype(y[b, (t / P) * P + p, c]),  p < P;   tok[.., p] = 0,  P <= p < ldp
//
//   delta [n_days, C, C] and bias [n_days, C] are fp32 masters, zero at init: a fresh adapter is exactly the identity and weight decay
//   pulls towards the identity.  No nonlinearity.  x is data (no gradient).  Products and sums are fp32 in both compute modes (the exact
//   fp32-input MFMA v_mfma_f32_32x32x2_f32 of vq.hip: a k-ordered fmaf chain from zero, to which x + bias is added once at the end: a
//   chain that STARTS at x + bias rounds every one of its C steps at the magnitude of the bias, which cost two bits at C = 256 and a
//   bias of 20), the only rounding to the compute dtype is the final store.  An out-of-range d selects a code path, it is never used as
//   an index.  With delta == 0 and bias == 0 the tokens have the values of fk_patchify.
//
//     d_delta[d, c, c'] = sum_{b: day[b] = d} sum_t x[b, t, c] * dy[b, t, c']        dy[b, tp * P + p, c'] = d_tok[b, tp * C + c', p]
//     d_bias[d, c']     = sum_{b: day[b] = d} sum_t dy[b, t, c']
//   all n_days slices are overwritten; a day absent from the batch gets exact zeros.
//
// fk_day_adapter_fwd: a workgroup owns 32 * G time steps of one sample (G = 1, 2, 4: more than one patch, so delta[d] is read once per
//   32 * G rows, from L2) and all C output channels.  The rows are staged in LDS ([32 G][Cp + 1] fp32, Cp = C rounded up to 32, tails
//   zero), time is the M side (x is the A operand, read from LDS), the output channel sits on the lane (delta is the B operand, read
//   from global memory, 32 consecutive floats per lane half and k).  Wave w holds the column tiles w, w + 4, ... as NCT * G accumulators
//   of 16 registers.  The results go back into the same LDS image and leave it transposed, p fastest, as in patchify_kernel: the adapted
//   [B, T, C] signal never exists in memory.
// fk_day_adapter_bwd: two launches, no atomics.  (1) a workgroup takes one (sample, time slice) and a 128 x 128 block of (c, c'):
//   32 rows of x and of dy (the un-patchify gather happens in the staging loop) at a time in LDS, wave w owns c rows 32 w .. 32 w + 31
//   and 4 column tiles; its sum goes to workspace[b][slice] (and the column sums of dy, four interleaved chains per 32 rows).  A sample
//   whose day is out of range writes nothing.  (2) every element of every day's slice adds the partials of the samples of that day in
//   (b, slice) order: every workgroup scans the B day ids itself.  The order depends on (B, T, C, P) and the contents of day only: same
//   bits on every run.  The number of slices is chosen from the shape alone so that one day for the whole batch still fills the chip.
#include "fk_common.h"

namespace {

constexpr int DA_TPB = 256;                  // 4 waves
constexpr int DA_LDS_FLOATS = 33 * 1024;     // forward LDS image: 32 G rows of Cp + 1 floats, at most 132 KiB
constexpr int DB_TILE = 128;                 // backward: (c, c') block per workgroup
constexpr int DB_ROWS = 32;                  // backward: time steps per LDS stage

struct DaFwdArgs {
  const float* x;
  const int64_t* day;
  const float* delta;
  const float* bias;
  void* tok;
  int B, T, C, P, ldp, n_days, Cp, ntile;
};

template <typename E, int NCT, int G>
__global__ __launch_bounds__(DA_TPB) void day_fwd_kernel(DaFwdArgs a) {
  extern __shared__ float xs[];              // [32 G][Cp + 1]
  constexpr int R = 32 * G;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
  const int C = a.C, Cp = a.Cp, ld = Cp + 1, P = a.P, ldp = a.ldp, T_ = a.T;
  const int b = blockIdx.x / a.ntile, t0 = (blockIdx.x % a.ntile) * R;
  const int rows = T_ - t0 < R ? T_ - t0 : R;
  const float* src = a.x + ((int64_t)b * T_ + t0) * C;
  for (int idx = tid; idx < R * Cp; idx += DA_TPB) {
    const int r = idx / Cp, c = idx - r * Cp;
    xs[r * ld + c] = (r < rows && c < C) ? src[(int64_t)r * C + c] : 0.0f;
  }
  __syncthreads();
  const int64_t d = a.day ? a.day[b] : -1;
  if (d >= 0 && d < a.n_days) {              // uniform over the workgroup
    const float* dl = a.delta + d * C * C;
    const float* bs = a.bias + d * C;
    f32x16 acc[NCT][G];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][g][r] = 0.0f;
    // 16 input channels (8 MFMA steps) per round; the delta values of the next round are in flight behind this round's MFMAs
    float bnext[NCT][8];
    auto load_delta = [&](int k0) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const int col = (ct * 4 + wave) * 32 + i;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int kk = k0 + 2 * s + h;
          bnext[ct][s] = (kk < C && col < C) ? dl[(int64_t)kk * C + col] : 0.0f;
        }
      }
    };
    load_delta(0);
    for (int k0 = 0; k0 < Cp; k0 += 16) {
      float bcur[NCT][8];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int s = 0; s < 8; ++s) bcur[ct][s] = bnext[ct][s];
      if (k0 + 16 < Cp) load_delta(k0 + 16);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int kk = k0 + 2 * s + h;
        float av[G];
#pragma unroll
        for (int g = 0; g < G; ++g) av[g] = xs[(g * 32 + i) * ld + kk];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          if ((ct * 4 + wave) * 32 < Cp) {   // uniform over the wave
#pragma unroll
            for (int g = 0; g < G; ++g) acc[ct][g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g], bcur[ct][s], acc[ct][g], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();                         // every wave has read its last x
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      if ((ct * 4 + wave) * 32 < Cp) {
        const int col = (ct * 4 + wave) * 32 + i;
        const float bv = col < C ? bs[col] : 0.0f;
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int r = 0; r < 16; ++r) {       // (x + bias) + sum: with delta == 0 the sum is +0 and x + bias comes through exactly
            float* q = xs + (g * 32 + acc_row(r, h)) * ld + col;
            *q = (*q + bv) + acc[ct][g][r];
          }
      }
    }
    __syncthreads();
  }
  // the patches these rows touch, transposed out of LDS: (patch, channel, p) with p fastest
  const int nT = T_ / P;
  const int tp0 = t0 / P, tp1 = (t0 + rows - 1) / P;
  E* tok = (E*)a.tok;
  const int per = C * ldp;
  const int total = (tp1 - tp0 + 1) * per;
  for (int idx = tid; idx < total; idx += DA_TPB) {
    const int q = idx / per, rem = idx - q * per;
    const int c = rem / ldp, p = rem - c * ldp;
    const int tp = tp0 + q;
    const int t = tp * P + (p < P ? p : P - 1) - t0;      // a pad column goes with the last row of its patch
    if (t < 0 || t >= rows) continue;
    tok[(((int64_t)b * nT + tp) * C + c) * ldp + p] = from_f32<E>(p < P ? xs[t * ld + c] : 0.0f);
  }
}

struct DaBwdArgs {
  const float* x;
  const int64_t* day;
  const float* d_tok;
  float* part;       // [B * S][C][C]
  float* partb;      // [B * S][C]
  float* d_delta;
  float* d_bias;
  int B, T, C, P, ldp, n_days, S, RS, ngrp;
};

__global__ __launch_bounds__(DA_TPB) void day_bwd_partial_kernel(DaBwdArgs a) {
  __shared__ float xS[DB_ROWS][DB_TILE + 1];
  __shared__ float dS[DB_ROWS][DB_TILE + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
  const int C = a.C, P = a.P, ldp = a.ldp, T_ = a.T, nT = T_ / P;
  const int chunk = blockIdx.x, b = chunk / a.S, s = chunk - b * a.S;
  const int gi = blockIdx.y / a.ngrp, gj = blockIdx.y - gi * a.ngrp;
  const int64_t d = a.day[b];
  if (d < 0 || d >= a.n_days) return;        // uniform: this sample's partials are never read
  const int t_lo = s * a.RS, t_hi = t_lo + a.RS < T_ ? t_lo + a.RS : T_;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
  float bsum = 0.0f;
  for (int tb = t_lo; tb < t_hi; tb += DB_ROWS) {
    __syncthreads();
    for (int idx = tid; idx < DB_ROWS * DB_TILE; idx += DA_TPB) {
      const int r = idx / DB_TILE, cl = idx - r * DB_TILE;
      const int t = tb + r, c = gi * DB_TILE + cl;
      xS[r][cl] = (t < t_hi && c < C) ? a.x[((int64_t)b * T_ + t) * C + c] : 0.0f;
    }
    for (int idx = tid; idx < DB_ROWS * DB_TILE; idx += DA_TPB) {
      const int cl = idx / DB_ROWS, r = idx - cl * DB_ROWS;
      const int t = tb + r, c = gj * DB_TILE + cl;
      float v = 0.0f;
      if (t < t_hi && c < C) {
        const int tp = t / P, p = t - tp * P;
        v = a.d_tok[(((int64_t)b * nT + tp) * C + c) * ldp + p];
      }
      dS[r][cl] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DB_ROWS; k += 2) {
      const float av = xS[k + h][wave * 32 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, dS[k + h][j * 32 + i], acc[j], 0, 0, 0);
    }
    if (gi == 0 && tid < DB_TILE) {          // column sums of dy: four interleaved chains per stage, then one chain over the stages
      float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < DB_ROWS; ++r) q[r & 3] += dS[r][tid];
      bsum += (q[0] + q[1]) + (q[2] + q[3]);
    }
  }
  float* part = a.part + (int64_t)chunk * C * C;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cc = gj * DB_TILE + j * 32 + i;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = gi * DB_TILE + wave * 32 + acc_row(r, h);
      if (c < C && cc < C) part[(int64_t)c * C + cc] = acc[j][r];
    }
  }
  if (gi == 0 && tid < DB_TILE && gj * DB_TILE + tid < C) a.partb[(int64_t)chunk * C + gj * DB_TILE + tid] = bsum;
}

// element e of day blockIdx.y: the partials of that day's samples in (b, slice) order; e < C * C: d_delta, then d_bias
__global__ __launch_bounds__(DA_TPB) void day_bwd_reduce_kernel(DaBwdArgs a) {
  const int C = a.C;
  const int64_t cc = (int64_t)C * C;
  const int64_t e = (int64_t)blockIdx.x * DA_TPB + threadIdx.x;
  const int64_t d = blockIdx.y;
  if (e >= cc + C) return;
  float sum = 0.0f;
  if (a.day) {
    for (int b = 0; b < a.B; ++b) {
      if (a.day[b] != d) continue;
      for (int s = 0; s < a.S; ++s) {
        const int64_t chunk = (int64_t)b * a.S + s;
        sum += e < cc ? a.part[chunk * cc + e] : a.partb[chunk * C + (e - cc)];
      }
    }
  }
  if (e < cc) a.d_delta[d * cc + e] = sum;
  else a.d_bias[d * C + (e - cc)] = sum;
}

// time slices per sample of the backward: enough (sample, slice, block) workgroups for the chip, at least 32 rows each
void bwd_split(int64_t B, int64_t T, int64_t C, int* S, int* RS, int* ngrp) {
  const int64_t g = fk_cdiv(C, DB_TILE);
  int64_t want = fk_cdiv(256, B * g * g);
  const int64_t most = fk_cdiv(T, DB_ROWS);
  if (want > most) want = most;
  if (want < 1) want = 1;
  const int64_t rs = fk_cdiv(fk_cdiv(T, want), DB_ROWS) * DB_ROWS;
  *RS = (int)rs;
  *S = (int)fk_cdiv(T, rs);
  *ngrp = (int)g;
}

int day_check(const char* name, int64_t B, int64_t T, int64_t C, int64_t P, int64_t ldp, int64_t n_days) {
  if (!(B > 0 && T > 0 && P > 0 && T % P == 0 && ldp >= P))
    return fk_set_error(FK_EINVAL, "%s: bad shape (B %lld, T %lld, P %lld, ldp %lld: T %% P must be 0, ldp >= P)", name, (long long)B, (long long)T,
                        (long long)P, (long long)ldp);
  if (!(C >= 1 && C <= 512)) return fk_set_error(FK_EINVAL, "%s: C = %lld outside the envelope 1 <= C <= 512", name, (long long)C);
  if (n_days < 1) return fk_set_error(FK_EINVAL, "%s: n_days = %lld, need at least one day", name, (long long)n_days);
  const int64_t lim = 1LL << 31;
  if (!(B < lim && T < lim && ldp < lim && n_days < lim && B * T < lim / C && B * (T / P) * C < lim / ldp && n_days * C * C < lim))
    return fk_set_error(FK_EINVAL, "%s: sizes exceed int32", name);
  return FK_OK;
}

// the kernel's LDS limit is raised once to the largest image any shape takes; each launch asks for its own
template <auto Kernel>
void day_fwd_go(const DaFwdArgs& a, int G, hipStream_t s) {
  static const bool once = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(DA_LDS_FLOATS * sizeof(float))) == hipSuccess;
  (void)once;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)(a.B * a.ntile)), dim3(DA_TPB), (size_t)32 * G * (a.Cp + 1) * sizeof(float), s, a);
}

template <typename E, int NCT>
void day_fwd_launch(const DaFwdArgs& a0, hipStream_t s) {
  DaFwdArgs a = a0;
  // the most rows per workgroup that fit the accumulators (NCT * G <= 8) and the LDS image and still leave a workgroup per CU
  int G = NCT == 4 ? 2 : 4;
  while (G > 1 && (32 * G * (a.Cp + 1) > DA_LDS_FLOATS || (int64_t)a.B * fk_cdiv(a.T, 32 * G) < 256)) G >>= 1;
  a.ntile = (int)fk_cdiv(a.T, 32 * G);
  if constexpr (NCT < 4) {
    if (G == 4) return day_fwd_go<day_fwd_kernel<E, NCT, 4>>(a, G, s);
  }
  if (G == 2) return day_fwd_go<day_fwd_kernel<E, NCT, 2>>(a, G, s);
  day_fwd_go<day_fwd_kernel<E, NCT, 1>>(a, 1, s);
}

}  // namespace

extern "C" {

int fk_day_adapter_fwd(const float* x, const int64_t* day, const float* delta, const float* bias, void* tok, int64_t B, int64_t T, int64_t C,
                       int64_t P, int64_t ldp, int64_t n_days, int dtype, void* stream) {
  FK_DT_CHECK("fk_day_adapter_fwd");
  FK_CHECK_ARG(x && tok && delta && bias, "fk_day_adapter_fwd: null pointer");
  if (int rc = day_check("fk_day_adapter_fwd", B, T, C, P, ldp, n_days)) return rc;
  FK_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)delta & 3) == 0 && ((uintptr_t)bias & 3) == 0 && ((uintptr_t)day & 7) == 0 &&
                   ((uintptr_t)tok & (dtype == FK_BF16 ? 1 : 3)) == 0,
               "fk_day_adapter_fwd: misaligned pointer");
  const int Cp = (int)(fk_cdiv(C, 32) * 32);
  const DaFwdArgs a{x, day, delta, bias, tok, (int)B, (int)T, (int)C, (int)P, (int)ldp, (int)n_days, Cp, 0};
  hipStream_t s = (hipStream_t)stream;
  if (C <= 128) FK_BY_DTYPE(dtype, E, day_fwd_launch<E, 1>(a, s));
  else if (C <= 256) FK_BY_DTYPE(dtype, E, day_fwd_launch<E, 2>(a, s));
  else FK_BY_DTYPE(dtype, E, day_fwd_launch<E, 4>(a, s));
  FK_CHECK_LAUNCH("fk_day_adapter_fwd");
  return FK_OK;
}

size_t fk_day_adapter_bwd_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t P, int64_t n_days) {
  if (B <= 0 || T <= 0 || C <= 0 || C > 512 || P <= 0 || n_days <= 0) return 0;
  int S, RS, ngrp;
  bwd_split(B, T, C, &S, &RS, &ngrp);
  return (size_t)B * S * (C * C + C) * sizeof(float);
}

int fk_day_adapter_bwd(const float* x, const int64_t* day, const float* d_tok, int64_t ldp, float* d_delta, float* d_bias, void* workspace,
                       size_t workspace_bytes, int64_t B, int64_t T, int64_t C, int64_t P, int64_t n_days, void* stream) {
  FK_CHECK_ARG(x && d_tok && d_delta && d_bias, "fk_day_adapter_bwd: null pointer");
  if (int rc = day_check("fk_day_adapter_bwd", B, T, C, P, ldp, n_days)) return rc;
  FK_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)d_tok & 3) == 0 && ((uintptr_t)d_delta & 3) == 0 && ((uintptr_t)d_bias & 3) == 0 &&
                   ((uintptr_t)day & 7) == 0 && ((uintptr_t)workspace & 3) == 0,
               "fk_day_adapter_bwd: misaligned pointer");
  int S, RS, ngrp;
  bwd_split(B, T, C, &S, &RS, &ngrp);
  FK_CHECK_ARG(B * S < (1LL << 31) / (C * C + C) && n_days <= 65535, "fk_day_adapter_bwd: sizes exceed int32 (or more than 65535 days)");
  FK_CHECK_ARG(!day || (workspace && workspace_bytes >= fk_day_adapter_bwd_workspace_bytes(B, T, C, P, n_days)), "fk_day_adapter_bwd: workspace too small");
  float* part = (float*)workspace;
  const DaBwdArgs a{x, day, d_tok, part, part ? part + (int64_t)B * S * C * C : nullptr, d_delta, d_bias, (int)B, (int)T, (int)C, (int)P, (int)ldp,
                    (int)n_days, S, RS, ngrp};
  hipStream_t s = (hipStream_t)stream;
  if (day) hipLaunchKernelGGL(day_bwd_partial_kernel, dim3((unsigned)(B * S), (unsigned)(ngrp * ngrp)), dim3(DA_TPB), 0, s, a);
  FK_CHECK_LAUNCH("fk_day_adapter_bwd(partials)");
  hipLaunchKernelGGL(day_bwd_reduce_kernel, dim3((unsigned)fk_cdiv(C * C + C, DA_TPB), (unsigned)n_days), dim3(DA_TPB), 0, s, a);
  FK_CHECK_LAUNCH("fk_day_adapter_bwd");
  return FK_OK;
}

}  // extern "C"
