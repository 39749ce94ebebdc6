// vq.hip — the vector quantiser of the VQ-VAE tokenizer (models/vq_brain.py: cosine-similarity codebook, straight-through estimator,
// commitment loss, EMA codebook with dead-code re-seeding, spherical k-means initialisation) as four entry points:
//   fk_vq_assign           idx[r] = argmax_j <x_r / |x_r|, e_j> (lowest index on an exact tie), q = e_idx, per-code counts and sums of
//                          the unit-norm rows, commitment-loss sum — one launch, no [R, K] similarity matrix
//   fk_vq_bwd              dx = dq + c * (x - q): straight-through and commitment gradient in one elementwise launch
//   fk_vq_codebook_update  the EMA step with dead-code re-seeding (two launches), or one k-means mean update, over the K codes
//   fk_vq_route            host only: is a (D, K, dtype) problem inside the envelope of fk_vq_assign
//
// fk_vq_assign is "row on the lane": the 32 codes of a chunk are the A operand of v_mfma_f32_32x32x2_f32, 32 data rows the B operand, so
// lane (i, h) owns data row i, its 16 accumulator registers are 16 different codes (ascending with the register index), and the running
// (best, index) is an in-lane compare with a strict > (a later code never replaces an equal earlier one).  The similarity is exact fp32
// whatever the dtype of x: bf16 rows are widened in registers and the codes are read as the fp32 buffer they are, so the indices depend
// on the values of x only.  Operand slots: lane half h holds the contiguous k range [h * DP / 2, (h + 1) * DP / 2) of its row (DP = D
// rounded up to 16 / 32 / 64 / 128, zero filled: fma(0, 0, acc) = acc), step s of a chunk multiplies slot s of both halves.
// The 8 waves of a workgroup split the chunks of the codebook (wave w: chunks w, w + 8, ...; the codebook is read from L2, 256 KiB at
// K = 1024, D = 64) and combine through LDS, preferring the larger value, then the lower index.  Code tails are masked to -inf, row
// tails are predicated.  The commitment sum is one partial per workgroup, each in a fixed order, added by the last workgroup to finish
// (ticket) in index order: the same bits on every run.  counts / sums use fp32 atomics like fk_scatter_add_rows.
#include "fk_common.h"

namespace {

constexpr int VQ_ROWS = 32;                  // data rows per workgroup
constexpr int VQ_CHUNK = 32;                 // codes per MFMA tile
constexpr int VQ_WAVES = 8;                  // waves per workgroup, each with its own chunks of the codebook
constexpr int VQ_TPB = 64 * VQ_WAVES;
constexpr int VQ_NONE = 0x7fffffff;          // "no code yet" (K < 2^31 keeps every real index below it)
constexpr int VQ_LDS = VQ_WAVES * 64 * 8 + VQ_ROWS * 8 + VQ_WAVES * 4;
static_assert(VQ_LDS <= 160 * 1024, "fk_vq_assign: LDS budget");

struct VqArgs {
  const void* x;
  int64_t ldx;
  const float* codes;
  int64_t* idx;
  void* q;
  float* counts;
  int64_t counts_stride;
  float* sums;
  int64_t ld_sums;
  float* partials;
  float* commit;
  float commit_scale;
  unsigned* ticket;
  int64_t R, K;
  int D;
};

template <typename T> FK_DEV f32x4 load4(const T* p);
template <> FK_DEV f32x4 load4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <> FK_DEV f32x4 load4<bf16_t>(const bf16_t* p) {
  const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
// v rounded to T, stored, and returned as the fp32 value of what was stored
template <typename T> FK_DEV f32x4 round4(const f32x4& v);
template <> FK_DEV f32x4 round4<float>(const f32x4& v) { return v; }
template <> FK_DEV f32x4 round4<bf16_t>(const f32x4& v) {
  return f32x4{(float)(bf16_t)v[0], (float)(bf16_t)v[1], (float)(bf16_t)v[2], (float)(bf16_t)v[3]};
}
template <typename T> FK_DEV void store4(T* p, const f32x4& v);
template <> FK_DEV void store4<float>(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
template <> FK_DEV void store4<bf16_t>(bf16_t* p, const f32x4& v) {
  *reinterpret_cast<bf16x4*>(p) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
}

template <typename T, int DP>
__global__ __launch_bounds__(VQ_TPB) void vq_assign_kernel(VqArgs a) {
  constexpr int H = DP / 2;                  // k slots per lane
  __shared__ float s_best[VQ_WAVES][64];
  __shared__ int s_bidx[VQ_WAVES][64];
  __shared__ float s_nrm[VQ_ROWS];
  __shared__ int s_idx[VQ_ROWS];
  __shared__ float s_red[VQ_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
  const int D = a.D;
  const int64_t row0 = (int64_t)blockIdx.x * VQ_ROWS;
  const T* x = (const T*)a.x;

  // B operand: this lane's half of data row i, normalised
  float b[H];
  {
    const int64_t row = row0 + i;
    const T* xp = x + row * a.ldx + h * H;
    float ss = 0.0f;
#pragma unroll
    for (int e = 0; e < H; e += 4) {
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (row < a.R && h * H + e < D) v = load4<T>(xp + e);
#pragma unroll
      for (int u = 0; u < 4; ++u) { b[e + u] = v[u]; ss = fmaf(v[u], v[u], ss); }
    }
    ss += __shfl_xor(ss, 32, 64);            // the other half of the row (a + b == b + a: both halves hold the same bits)
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int e = 0; e < H; ++e) b[e] = b[e] / nrm;
    if (wave == 0 && h == 0) s_nrm[i] = nrm;
  }

  float best = -INFINITY;
  int bi = VQ_NONE;
  const int64_t nchunk = (a.K + VQ_CHUNK - 1) / VQ_CHUNK;
  for (int64_t c = wave; c < nchunk; c += VQ_WAVES) {
    const int64_t code = c * VQ_CHUNK + i;   // the A row of this lane
    const float* cp = a.codes + code * D + h * H;
    float av[H];
#pragma unroll
    for (int e = 0; e < H; e += 4) {
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (code < a.K && h * H + e < D) v = *reinterpret_cast<const f32x4*>(cp + e);
#pragma unroll
      for (int u = 0; u < 4; ++u) av[e + u] = v[u];
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < H; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], b[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {           // acc_row() ascends with r: a strict > keeps the lowest index
      const int64_t cj = c * VQ_CHUNK + acc_row(r, h);
      const float v = cj < a.K ? acc[r] : -INFINITY;
      if (v > best) { best = v; bi = (int)cj; }
    }
  }
  s_best[wave][lane] = best;
  s_bidx[wave][lane] = bi;
  __syncthreads();
  if (threadIdx.x < VQ_ROWS) {
    float bb = -INFINITY;
    int bj = VQ_NONE;
#pragma unroll
    for (int w = 0; w < VQ_WAVES; ++w)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const float v = s_best[w][hh * 32 + threadIdx.x];
        const int j = s_bidx[w][hh * 32 + threadIdx.x];
        if (v > bb || (v == bb && j < bj)) { bb = v; bj = j; }
      }
    if (bj == VQ_NONE) bj = 0;               // a row of NaNs: index 0, as fk_argmax_rows
    s_idx[threadIdx.x] = bj;
    if (row0 + threadIdx.x < a.R) {
      a.idx[row0 + threadIdx.x] = bj;
      if (a.counts) atomicAdd(a.counts + (int64_t)bj * a.counts_stride, 1.0f);
    }
  }
  if (!a.q && !a.sums && !a.partials) return;
  __syncthreads();

  // epilogue over the 32 x D tile: q = round(e_idx), sum (x - q)^2, sums[idx] += x / |x|
  const int d4 = D >> 2;
  float part = 0.0f;
  for (int it = threadIdx.x; it < VQ_ROWS * d4; it += VQ_TPB) {
    const int r = it / d4, k = (it - r * d4) << 2;
    const int64_t row = row0 + r;
    if (row >= a.R) break;
    const int64_t j = s_idx[r];
    const f32x4 xv = load4<T>(x + row * a.ldx + k);
    const f32x4 qv = round4<T>(*reinterpret_cast<const f32x4*>(a.codes + j * D + k));
    if (a.q) store4<T>((T*)a.q + row * D + k, qv);
    if (a.partials) {
#pragma unroll
      for (int u = 0; u < 4; ++u) { const float d = xv[u] - qv[u]; part = fmaf(d, d, part); }
    }
    if (a.sums) {
      const float nrm = s_nrm[r];
#pragma unroll
      for (int u = 0; u < 4; ++u) atomicAdd(a.sums + j * a.ld_sums + k + u, xv[u] / nrm);
    }
  }
  if (!a.partials) return;
  part = wave_sum(part);
  if (lane == 0) s_red[wave] = part;
  __syncthreads();
  if (wave != 0) return;
  unsigned last = 0u;
  if (lane == 0) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < VQ_WAVES; ++w) t += s_red[w];
    __hip_atomic_store(a.partials + blockIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  last = __shfl(last, 0, 64);
  if (!last) return;
  // the last workgroup: every partial is in memory; lane l adds partials l, l + 64, ... in order, then one xor tree
  __threadfence();
  float t = 0.0f;
  for (unsigned p = lane; p < gridDim.x; p += 64) t += __hip_atomic_load(a.partials + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  t = wave_sum(t);
  if (lane == 0) {
    a.commit[0] = t * a.commit_scale;
    atomicExch(a.ticket, 0u);
  }
}

template <typename T>
__global__ void vq_bwd_kernel(const T* x, const T* q, const T* dq, const float* d_commit, float c_scale, T* dx, int64_t n) {
  const float c = d_commit ? d_commit[0] * c_scale : 0.0f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float g = dq ? to_f32<T>(dq[i]) : 0.0f;
    dx[i] = from_f32<T>(fmaf(c, to_f32<T>(x[i]) - to_f32<T>(q[i]), g));
  }
}

constexpr int VU_TPB = 1024;
constexpr int VU_GROUP = 16;                 // lanes per code
struct VuArgs {
  float* embed;
  float* embed_avg;
  float* cluster_size;
  const float* counts;
  int64_t counts_stride;
  const float* sums;
  int64_t ld_sums;
  const float* seed;
  int64_t K;
  int D;
  float decay, eps, dead;
  int mode;
  float* n_ws;
};

FK_DEV float group_sum(float v) {
#pragma unroll
  for (int o = VU_GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// EMA mode, first launch (ONE workgroup: n = the sum of the K new cluster sizes is needed by every code, and cluster_size is updated in
// place): cs = decay * cs + (1 - decay) * counts, n_ws[0] = sum cs in a fixed order.
__global__ __launch_bounds__(VU_TPB) void vq_cluster_size_kernel(VuArgs a) {
  __shared__ float s_red[VU_TPB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float omd = 1.0f - a.decay;
  float part = 0.0f;
  for (int64_t j = tid; j < a.K; j += VU_TPB) {
    const float c = a.decay * a.cluster_size[j] + omd * a.counts[j * a.counts_stride];
    a.cluster_size[j] = c;
    part += c;
  }
  part = wave_sum(part);
  if (lane == 0) s_red[wave] = part;
  __syncthreads();
  if (tid == 0) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < VU_TPB / 64; ++w) t += s_red[w];
    a.n_ws[0] = t;
  }
}

// The codes, 16 lanes each (second launch of the EMA mode, the only one of the k-means mode): a workgroup touches its own codes only.
__global__ __launch_bounds__(VU_TPB) void vq_codebook_update_kernel(VuArgs a) {
  const int tid = threadIdx.x;
  const int D = a.D;
  const float omd = 1.0f - a.decay;
  const float n = a.mode == FK_VQ_EMA ? a.n_ws[0] : 0.0f;
  const int gl = tid & (VU_GROUP - 1);
  const int64_t ngroups = (int64_t)gridDim.x * (VU_TPB / VU_GROUP);
  for (int64_t j = (int64_t)blockIdx.x * (VU_TPB / VU_GROUP) + tid / VU_GROUP; j < a.K; j += ngroups) {
    float* e = a.embed + j * D;
    const float* sm = a.sums + j * a.ld_sums;
    if (a.mode == FK_VQ_KMEANS) {
      const float cnt = a.counts[j * a.counts_stride];
      if (!(cnt > 0.0f)) continue;           // an empty cluster keeps its mean
      float ss = 0.0f;
      for (int k = gl; k < D; k += VU_GROUP) { const float v = sm[k] / cnt; ss = fmaf(v, v, ss); }
      const float nrm = fmaxf(sqrtf(group_sum(ss)), 1e-12f);
      for (int k = gl; k < D; k += VU_GROUP) e[k] = sm[k] / cnt / nrm;
      continue;
    }
    const float c = a.cluster_size[j];
    float* avg = a.embed_avg + j * D;
    if (c < a.dead) {                        // re-seed: embed = seed / |seed|, embed_avg = embed * dead, cluster_size = dead
      const float* sd = a.seed + j * D;
      float ss = 0.0f;
      for (int k = gl; k < D; k += VU_GROUP) ss = fmaf(sd[k], sd[k], ss);
      const float nrm = fmaxf(sqrtf(group_sum(ss)), 1e-12f);
      for (int k = gl; k < D; k += VU_GROUP) {
        const float v = sd[k] / nrm;
        e[k] = v;
        avg[k] = v * a.dead;
      }
      if (gl == 0) a.cluster_size[j] = a.dead;
      continue;
    }
    const float smoothed = (c + a.eps) / (n + (float)a.K * a.eps) * n;
    float ss = 0.0f;
    for (int k = gl; k < D; k += VU_GROUP) {
      const float v = (a.decay * avg[k] + omd * sm[k]) / smoothed;
      ss = fmaf(v, v, ss);
    }
    const float nrm = fmaxf(sqrtf(group_sum(ss)), 1e-12f);
    for (int k = gl; k < D; k += VU_GROUP) {
      const float av = a.decay * avg[k] + omd * sm[k];
      avg[k] = av;
      e[k] = av / smoothed / nrm;
    }
  }
}

bool vq_fused(int64_t D, int64_t K, int dtype) {
  return (dtype == FK_F32 || dtype == FK_BF16) && D >= 4 && D <= 128 && D % 4 == 0 && K >= 1 && K < (1LL << 31);
}

template <typename T>
void vq_assign_launch(const VqArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)fk_cdiv(a.R, VQ_ROWS)), block(VQ_TPB);
  if (a.D <= 16) hipLaunchKernelGGL((vq_assign_kernel<T, 16>), grid, block, 0, s, a);
  else if (a.D <= 32) hipLaunchKernelGGL((vq_assign_kernel<T, 32>), grid, block, 0, s, a);
  else if (a.D <= 64) hipLaunchKernelGGL((vq_assign_kernel<T, 64>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((vq_assign_kernel<T, 128>), grid, block, 0, s, a);
}

}  // namespace

extern "C" {

int fk_vq_route(int64_t D, int64_t K, int dtype) { return vq_fused(D, K, dtype) ? FK_VQ_FUSED : FK_VQ_CHAIN; }

int fk_vq_assign(const void* x, int64_t ldx, const float* codes, int64_t* idx, void* q, float* counts, int64_t counts_stride, float* sums,
                 int64_t ld_sums, float* commit_partials, float* commit, float commit_scale, uint32_t* ticket, int64_t R, int64_t K,
                 int64_t D, int dtype, void* stream) {
  FK_DT_CHECK("fk_vq_assign");
  FK_CHECK_ARG(x && codes && idx, "fk_vq_assign: null pointer");
  FK_CHECK_ARG(R > 0 && R < (1LL << 36) && K > 0 && D > 0 && ldx >= D, "fk_vq_assign: bad shape (R %lld, K %lld, D %lld, ldx %lld)", (long long)R,
               (long long)K, (long long)D, (long long)ldx);
  FK_CHECK_ARG(!counts || counts_stride >= 1, "fk_vq_assign: counts_stride");
  FK_CHECK_ARG(!sums || ld_sums >= D, "fk_vq_assign: ld_sums shorter than a row");
  FK_CHECK_ARG((commit_partials != nullptr) == (commit != nullptr) && (commit != nullptr) == (ticket != nullptr),
               "fk_vq_assign: commit_partials, commit and ticket go together");
  const int64_t xal = dtype == FK_BF16 ? 7 : 15;
  FK_CHECK_ARG(((uintptr_t)x & xal) == 0 && ldx % 4 == 0 && ((uintptr_t)codes & 15) == 0 && (!q || ((uintptr_t)q & xal) == 0),
               "fk_vq_assign: x / q rows must be aligned to 4 elements, codes to 16 bytes");
  if (!vq_fused(D, K, dtype)) return fk_set_error(FK_EUNSUPPORTED, "fk_vq_assign: outside the envelope (D %% 4 == 0, 4 <= D <= 128, K < 2^31): see fk_vq_route");
  const VqArgs a{x, ldx, codes, idx, q, counts, counts_stride, sums, ld_sums, commit_partials, commit, commit_scale, ticket, R, K, (int)D};
  FK_BY_DTYPE(dtype, T, vq_assign_launch<T>(a, (hipStream_t)stream));
  FK_CHECK_LAUNCH("fk_vq_assign");
  return FK_OK;
}

int fk_vq_bwd(const void* x, const void* q, const void* dq, const float* d_commit, float c_scale, void* dx, int64_t n, int dtype,
              void* stream) {
  FK_DT_CHECK("fk_vq_bwd");
  FK_CHECK_ARG(x && q && dx && n > 0, "fk_vq_bwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (unsigned)(fk_cdiv(n, 256) < 65536 ? fk_cdiv(n, 256) : 65536);
  FK_BY_DTYPE(dtype, T, hipLaunchKernelGGL(vq_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)x, (const T*)q, (const T*)dq, d_commit, c_scale, (T*)dx, n));
  FK_CHECK_LAUNCH("fk_vq_bwd");
  return FK_OK;
}

int fk_vq_codebook_update(float* embed, float* embed_avg, float* cluster_size, const float* counts, int64_t counts_stride,
                          const float* sums, int64_t ld_sums, const float* seed, float* n_ws, int64_t K, int64_t D, float decay, float eps,
                          float dead, int mode, void* stream) {
  FK_CHECK_ARG(mode == FK_VQ_EMA || mode == FK_VQ_KMEANS, "fk_vq_codebook_update: bad mode %d", mode);
  FK_CHECK_ARG(embed && counts && sums, "fk_vq_codebook_update: null pointer");
  FK_CHECK_ARG(mode == FK_VQ_KMEANS || (embed_avg && cluster_size && seed && n_ws), "fk_vq_codebook_update: the EMA mode needs embed_avg, cluster_size, seed and n_ws");
  FK_CHECK_ARG(K > 0 && D > 0 && D < (1LL << 31) && counts_stride >= 1 && ld_sums >= D, "fk_vq_codebook_update: bad shape");
  const VuArgs a{embed, embed_avg, cluster_size, counts, counts_stride, sums, ld_sums, seed, K, (int)D, decay, eps, dead, mode, n_ws};
  const int64_t per = VU_TPB / VU_GROUP;
  const unsigned nb = (unsigned)(fk_cdiv(K, per) < 1024 ? fk_cdiv(K, per) : 1024);
  if (mode == FK_VQ_EMA) hipLaunchKernelGGL(vq_cluster_size_kernel, dim3(1), dim3(VU_TPB), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(vq_codebook_update_kernel, dim3(nb), dim3(VU_TPB), 0, (hipStream_t)stream, a);
  FK_CHECK_LAUNCH("fk_vq_codebook_update");
  return FK_OK;
}

}  // extern "C"
