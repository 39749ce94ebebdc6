// editdist.hip — unit-cost Levenshtein distance on int64 ids and the thin layers over it: error counts against a reference, all pairwise
// distances inside an n-best list, minimum-Bayes-risk ranking of the list and the terms of the minimum-word-error-rate loss.
// Semantics: include/franken_hip.h ("edit distance"); tests/edit_ref.py restates them in Python ints / float64.
//
//   lev_wave<R>                 ONE wave per pair, written once for both distance kernels.  The sequence x (at most 64 R tokens) sits on the
//                               lanes, R consecutive DP rows per lane in registers; the sequence y is staged once into LDS as int64 (ids are
//                               compared whole, never truncated).  The wave sweeps anti-diagonals: in step s lane l fills column s - l of its R
//                               rows, which needs the cell above its first row (lane l - 1's last row, one step old: ONE __shfl_up by one lane
//                               per step, the idiom of the wave route of ctc.hip), the one left of it (its own register) and the diagonal one
//                               (the value shuffled in one step earlier).  k + ceil(m / R) - 1 steps for lengths m, k; no min-scan anywhere.
//   fk_edit_distance            B groups x n pairs, the group's a sequence against n (n_a = 1) or pairwise (n_a = n)
//   fk_nbest_pairwise_distance  the pairs i <= j of every sentence, mirrored; -1 in the row and column of an empty beam slot
//   fk_mbr_rank                 one wave per sentence: posterior, expected distance in a fixed order, ranking by counting, gather
//   fk_mwer_combine             one workgroup for the batch (a thread per sentence): softmax(-nll), loss terms, d loss / d nll, sentence count
//   fk_mwer_reduce_rows         the gradient of the expanded logits back to the logits: the valid rows of a sentence added in a fixed order
// int32 distances, fp32 elsewhere, no atomics, no workspace, the same bits every run; nothing waits for the host.
#include "fk_common.h"

#include <math.h>

namespace {

constexpr int ED_MAX_HYPS = FK_NBEST_MAX_HYPS;
constexpr int ED_MAX_T = FK_NBEST_MAX_T;
static_assert(ED_MAX_T <= 64 * 16, "the widest route holds 16 rows per lane");
static_assert(ED_MAX_T * sizeof(int64_t) <= 64 * 1024, "the staged sequence fits the LDS every kernel may have");

// length of the sequence p[0 .. L): *lenp clamped into [0, L], or (lenp NULL) the position of the first `pad`, L without one.  Whole wave.
FK_DEV int seq_len(const int64_t* p, int L, const int64_t* lenp, int64_t pad, int lane) {
  if (lenp) {
    const int64_t l = *lenp;
    return (int)(l < 0 ? 0 : (l > L ? L : l));
  }
  for (int base = 0; base < L; base += 64) {
    const int j = base + lane;
    const bool hit = j < L && p[j] == pad;
    const unsigned long long mk = __ballot(hit);
    if (mk) return base + __ffsll((long long)mk) - 1;
  }
  return L;
}

// Levenshtein distance of x[0 .. m) and y[0 .. k), m <= 64 R, k <= ED_MAX_T, by the whole (single-wave) workgroup; every lane returns it.
// Entries at or behind m / k are never read.  s_y: k int64 of LDS.
template <int R>
FK_DEV int lev_wave(const int64_t* x, int m, const int64_t* y, int k, int64_t* s_y, int lane) {
  if (m == 0 || k == 0) return m + k;                                   // uniform
  for (int j = lane; j < k; j += 64) s_y[j] = y[j];
  __syncthreads();
  int64_t xr[R];
  int d[R];                                                             // D[row][column already done], row = lane R + r + 1
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane * R + r;
    xr[r] = i < m ? x[i] : 0;
    d[r] = i + 1;                                                       // column 0
  }
  int diag = lane * R;                                                  // D[lane R][column - 1]
  const int steps = k + (m + R - 1) / R - 1;
  for (int s = 0; s < steps; ++s) {
    const int c = s - lane;                                             // this lane's column (0-based token of y)
    const bool act = c >= 0 && c < k;
    int up = __shfl_up(d[R - 1], 1, 64);                                // D[lane R][c + 1]: the lane above filled that column one step ago
    if (lane == 0) up = c + 1;
    const int64_t yt = s_y[act ? c : 0];
    int above = up, dg = diag;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int left = d[r];
      const int ins = (left < above ? left : above) + 1;
      const int sub = dg + (xr[r] != yt ? 1 : 0);
      const int v = ins < sub ? ins : sub;
      dg = left;
      above = act ? v : left;
      d[r] = above;
    }
    diag = act ? up : diag;
  }
  const int last = m - 1;
  int sel = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) sel = (last % R) == r ? d[r] : sel;
  return __shfl(sel, last / R, 64);
}

struct EditArgs {
  const int64_t *a, *alen, *b, *blen;
  int64_t ld_a_b, ld_a_h, ld_b_b, ld_b_h, pad;
  int n_a, n, La, Lb;
  int32_t *dist, *alen_out;
};

// A_LANES: a is the narrower array and sits on the lanes
template <int R, bool A_LANES>
__global__ __launch_bounds__(64) void edit_distance_kernel(EditArgs a) {
  extern __shared__ int64_t ed_sy[];
  const int lane = threadIdx.x;
  const int64_t pair = blockIdx.x;
  const int64_t g = pair / a.n;
  const int h = (int)(pair - g * a.n), ha = a.n_a == 1 ? 0 : h;
  const int64_t* pa = a.a + g * a.ld_a_b + ha * a.ld_a_h;
  const int64_t* pb = a.b + g * a.ld_b_b + h * a.ld_b_h;
  const int la = seq_len(pa, a.La, a.alen ? a.alen + g * a.n_a + ha : nullptr, a.pad, lane);
  const int lb = seq_len(pb, a.Lb, a.blen ? a.blen + pair : nullptr, a.pad, lane);
  const int d = A_LANES ? lev_wave<R>(pa, la, pb, lb, ed_sy, lane) : lev_wave<R>(pb, lb, pa, la, ed_sy, lane);
  if (lane == 0) {
    a.dist[pair] = d;
    if (a.alen_out && (a.n_a != 1 || h == 0)) a.alen_out[g * a.n_a + ha] = la;
  }
}

struct PairArgs {
  const int64_t *ids, *lengths; const float* scores;
  int64_t ldb, ldh;
  int n, T;
  int32_t* dist;
};

template <int R>
__global__ __launch_bounds__(64) void nbest_pairwise_kernel(PairArgs a) {
  extern __shared__ int64_t ed_sy[];
  const int lane = threadIdx.x, n = a.n;
  const int per = n * (n + 1) / 2;
  const int64_t b = blockIdx.x / per;
  int p = (int)(blockIdx.x - b * per), i = 0;
  while (p >= n - i) { p -= n - i; ++i; }                               // pair number -> (i, j), i <= j
  const int j = i + p;
  const bool ok = !a.scores || (isfinite(a.scores[b * n + i]) && isfinite(a.scores[b * n + j]));
  int d = -1;
  if (ok && i == j) d = 0;
  if (ok && i != j) {                                                   // uniform
    const int64_t* x = a.ids + b * a.ldb + i * a.ldh;
    const int64_t* y = a.ids + b * a.ldb + j * a.ldh;
    const int m = seq_len(x, a.T, a.lengths + b * n + i, 0, lane), k = seq_len(y, a.T, a.lengths + b * n + j, 0, lane);
    d = lev_wave<R>(x, m, y, k, ed_sy, lane);
  }
  if (lane == 0) {
    int32_t* out = a.dist + b * n * n;
    out[i * n + j] = d;
    out[j * n + i] = d;
  }
}

struct MbrArgs {
  const int32_t* dist; const float* scores; float scale;
  const int64_t* ids; int64_t ldb, ldh; const int64_t* lengths;
  int n, T; int64_t pad;
  float* risk; int64_t *ids_out, *len_out; float *scores_out, *risk_out; int64_t *order, *n_valid;
};

__global__ __launch_bounds__(64) void mbr_rank_kernel(MbrArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
  __shared__ float s_sc[ED_MAX_HYPS], s_t[ED_MAX_HYPS], s_w[ED_MAX_HYPS], s_risk[ED_MAX_HYPS];
  __shared__ int s_ok[ED_MAX_HYPS], s_len[ED_MAX_HYPS], s_rank[ED_MAX_HYPS];
  if (tid < n) {
    const float sc = a.scores[(int64_t)b * n + tid];
    const int64_t l = a.lengths[(int64_t)b * n + tid];
    s_sc[tid] = sc;
    s_ok[tid] = isfinite(sc) ? 1 : 0;
    s_t[tid] = __fmul_rn(a.scale, sc);
    s_len[tid] = (int)(l < 0 ? 0 : (l > a.T ? a.T : l));
  }
  __syncthreads();
  float m = -INFINITY;
  int cnt = 0;
  for (int j = 0; j < n; ++j)
    if (s_ok[j]) { m = fmaxf(m, s_t[j]); ++cnt; }
  if (tid < n) s_w[tid] = s_ok[tid] ? expf(__fsub_rn(s_t[tid], m)) : 0.0f;
  __syncthreads();
  float Z = 0.0f;
  for (int j = 0; j < n; ++j)
    if (s_ok[j]) Z = __fadd_rn(Z, s_w[j]);
  if (tid < n) {
    float r = INFINITY;
    if (s_ok[tid]) {
      const int32_t* row = a.dist + ((int64_t)b * n + tid) * n;
      r = 0.0f;
      for (int j = 0; j < n; ++j)
        if (s_ok[j]) r = __fadd_rn(r, __fmul_rn(__fdiv_rn(s_w[j], Z), (float)row[j]));
    }
    s_risk[tid] = r;
    a.risk[(int64_t)b * n + tid] = r;
  }
  __syncthreads();
  if (tid < n) {
    const int h = tid;
    int rank = 0;
    for (int g = 0; g < n; ++g) {
      if (g == h) continue;
      bool beats;
      if (s_ok[g] != s_ok[h]) beats = s_ok[g] != 0;
      else if (!s_ok[g]) beats = g < h;
      else beats = s_risk[g] < s_risk[h] || (!(s_risk[h] < s_risk[g]) && g < h);
      rank += beats ? 1 : 0;
    }
    s_rank[h] = rank;
    const int64_t o = (int64_t)b * n + rank;
    a.len_out[o] = s_len[h]; a.scores_out[o] = s_sc[h]; a.risk_out[o] = s_risk[h]; a.order[o] = h;
    if (h == 0) a.n_valid[b] = cnt;
  }
  __syncthreads();
  const int64_t* ids = a.ids + (int64_t)b * a.ldb;
  int64_t* out = a.ids_out + (int64_t)b * n * a.T;
  for (int idx = tid; idx < n * a.T; idx += 64) {
    const int h = idx / a.T, j = idx - h * a.T;
    out[(int64_t)s_rank[h] * a.T + j] = j < s_len[h] ? ids[(int64_t)h * a.ldh + j] : a.pad;
  }
}

struct MwerArgs {
  const float* nll; const int32_t* errors; const float* scores; const int64_t* lengths; int64_t max_len;
  int B, n;
  float *loss, *coef, *count; uint8_t* valid;
};

constexpr int MW_THREADS = 256;

__global__ __launch_bounds__(MW_THREADS) void mwer_combine_kernel(MwerArgs a) {
  const int tid = threadIdx.x, n = a.n;
  __shared__ int s_cnt[MW_THREADS];
  int have = 0;
  for (int b = tid; b < a.B; b += MW_THREADS) {
    const float* nll = a.nll + (int64_t)b * n;
    const int32_t* err = a.errors + (int64_t)b * n;
    float* coef = a.coef + (int64_t)b * n;
    unsigned ok = 0;                                                    // n <= 32: a bit per hypothesis
    float m = -INFINITY;
    int cnt = 0, esum = 0;
    for (int i = 0; i < n; ++i) {
      const bool v = isfinite(nll[i]) && (!a.scores || isfinite(a.scores[(int64_t)b * n + i])) &&
                     (!a.lengths || a.lengths[(int64_t)b * n + i] <= a.max_len);
      if (a.valid) a.valid[(int64_t)b * n + i] = v ? 1 : 0;
      if (v) { ok |= 1u << i; m = fmaxf(m, -nll[i]); ++cnt; esum += err[i]; }
    }
    float loss = 0.0f;
    if (cnt) {
      float Z = 0.0f;
      for (int i = 0; i < n; ++i)
        if (ok >> i & 1u) Z = __fadd_rn(Z, expf(__fsub_rn(-nll[i], m)));
      const float ebar = __fdiv_rn((float)esum, (float)cnt);
      float pe = 0.0f;
      for (int i = 0; i < n; ++i)
        if (ok >> i & 1u) {
          const float p = __fdiv_rn(expf(__fsub_rn(-nll[i], m)), Z);
          pe = __fadd_rn(pe, __fmul_rn(p, (float)err[i]));
          loss = __fadd_rn(loss, __fmul_rn(p, __fsub_rn((float)err[i], ebar)));
        }
      for (int i = 0; i < n; ++i) {
        const float p = (ok >> i & 1u) ? __fdiv_rn(expf(__fsub_rn(-nll[i], m)), Z) : 0.0f;
        coef[i] = (ok >> i & 1u) ? -__fmul_rn(p, __fsub_rn((float)err[i], pe)) : 0.0f;
      }
      ++have;
    } else {
      for (int i = 0; i < n; ++i) coef[i] = 0.0f;
    }
    a.loss[b] = loss;
  }
  s_cnt[tid] = have;
  __syncthreads();
  for (int o = MW_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s_cnt[tid] += s_cnt[tid + o];
    __syncthreads();
  }
  if (tid == 0) a.count[0] = (float)s_cnt[0];
}

// out[b, e] (+)= sum over the valid i of rows[b n + i, e], added in ascending i in fp32
template <typename T>
__global__ void mwer_reduce_rows_kernel(const T* rows, const uint8_t* valid, T* out, int B, int n, int64_t E, int accumulate) {
  const int64_t total = (int64_t)B * E;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / E, e = idx - b * E;
    float acc = accumulate ? to_f32<T>(out[idx]) : 0.0f;
    for (int i = 0; i < n; ++i)
      if (valid[b * n + i]) acc += to_f32<T>(rows[(b * n + i) * E + e]);
    out[idx] = from_f32<T>(acc);
  }
}

int edit_route(int64_t La, int64_t Lb) {
  const int64_t m = La < Lb ? La : Lb;
  if (m < 1 || La > ED_MAX_T || Lb > ED_MAX_T) return -1;
  return m <= 64 ? FK_EDIT_LANE : (m <= 256 ? FK_EDIT_ROWS4 : FK_EDIT_ROWS16);
}

// one launch of K<R, ...> for the route's R
#define ED_BY_ROUTE(route, R, ...)                                      \
  do {                                                                  \
    if ((route) == FK_EDIT_LANE) { constexpr int R = 1; __VA_ARGS__; }  \
    else if ((route) == FK_EDIT_ROWS4) { constexpr int R = 4; __VA_ARGS__; } \
    else { constexpr int R = 16; __VA_ARGS__; }                         \
  } while (0)

}  // namespace

int fk_edit_distance_route(int64_t La, int64_t Lb) {
  const int r = edit_route(La, Lb);
  if (r < 0) return fk_set_error(FK_EINVAL, "fk_edit_distance_route: La = %lld, Lb = %lld outside the envelope (1 .. %d)", (long long)La, (long long)Lb, ED_MAX_T);
  return r;
}

int fk_edit_distance(const int64_t* a, int64_t ld_a_b, int64_t ld_a_h, const int64_t* alen, int64_t n_a, int64_t La, const int64_t* b, int64_t ld_b_b,
                     int64_t ld_b_h, const int64_t* blen, int64_t Lb, int64_t B, int64_t n, int64_t pad_value, int32_t* dist, int32_t* alen_out,
                     void* stream) {
  FK_CHECK_ARG(a && b && dist, "fk_edit_distance: null pointer");
  FK_CHECK_ARG(n >= 1 && n <= FK_NBEST_MAX_HYPS, "fk_edit_distance: n = %lld outside the envelope (1 .. %d)", (long long)n, FK_NBEST_MAX_HYPS);
  FK_CHECK_ARG(n_a == 1 || n_a == n, "fk_edit_distance: n_a = %lld is neither 1 nor n = %lld", (long long)n_a, (long long)n);
  FK_CHECK_ARG(La >= 1 && La <= FK_NBEST_MAX_T && Lb >= 1 && Lb <= FK_NBEST_MAX_T, "fk_edit_distance: La = %lld, Lb = %lld outside the envelope (1 .. %d)",
               (long long)La, (long long)Lb, FK_NBEST_MAX_T);
  FK_CHECK_ARG(B > 0 && B * n < (1LL << 31), "fk_edit_distance: B = %lld", (long long)B);
  FK_CHECK_ARG(ld_a_h >= La && ld_a_b >= (n_a - 1) * ld_a_h + La, "fk_edit_distance: a strides %lld / %lld below [n_a = %lld, La = %lld]",
               (long long)ld_a_b, (long long)ld_a_h, (long long)n_a, (long long)La);
  FK_CHECK_ARG(ld_b_h >= Lb && ld_b_b >= (n - 1) * ld_b_h + Lb, "fk_edit_distance: b strides %lld / %lld below [n = %lld, Lb = %lld]",
               (long long)ld_b_b, (long long)ld_b_h, (long long)n, (long long)Lb);
  EditArgs g;
  g.a = a; g.alen = alen; g.b = b; g.blen = blen; g.ld_a_b = ld_a_b; g.ld_a_h = ld_a_h; g.ld_b_b = ld_b_b; g.ld_b_h = ld_b_h; g.pad = pad_value;
  g.n_a = (int)n_a; g.n = (int)n; g.La = (int)La; g.Lb = (int)Lb; g.dist = dist; g.alen_out = alen_out;
  const bool a_lanes = La <= Lb;
  const size_t lds = sizeof(int64_t) * (size_t)(a_lanes ? Lb : La);
  const dim3 grid((unsigned)(B * n));
  ED_BY_ROUTE(edit_route(La, Lb), R, {
    if (a_lanes) hipLaunchKernelGGL((edit_distance_kernel<R, true>), grid, dim3(64), lds, (hipStream_t)stream, g);
    else hipLaunchKernelGGL((edit_distance_kernel<R, false>), grid, dim3(64), lds, (hipStream_t)stream, g);
  });
  FK_CHECK_LAUNCH("fk_edit_distance");
  return FK_OK;
}

int fk_nbest_pairwise_distance(const int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, const int64_t* lengths, const float* scores, int64_t B, int64_t n,
                               int64_t T, int32_t* dist, void* stream) {
  FK_CHECK_ARG(ids && lengths && dist, "fk_nbest_pairwise_distance: null pointer");
  FK_CHECK_ARG(n >= 1 && n <= FK_NBEST_MAX_HYPS, "fk_nbest_pairwise_distance: n = %lld hypotheses outside the envelope (1 .. %d)", (long long)n,
               FK_NBEST_MAX_HYPS);
  FK_CHECK_ARG(T >= 1 && T <= FK_NBEST_MAX_T, "fk_nbest_pairwise_distance: T = %lld outside the envelope (1 .. %d)", (long long)T, FK_NBEST_MAX_T);
  FK_CHECK_ARG(B > 0 && B * (n * (n + 1) / 2) < (1LL << 31), "fk_nbest_pairwise_distance: B = %lld", (long long)B);
  FK_CHECK_ARG(ld_ids_h >= T && ld_ids_b >= (n - 1) * ld_ids_h + T, "fk_nbest_pairwise_distance: ids strides %lld / %lld below [n = %lld, T = %lld]",
               (long long)ld_ids_b, (long long)ld_ids_h, (long long)n, (long long)T);
  PairArgs g;
  g.ids = ids; g.lengths = lengths; g.scores = scores; g.ldb = ld_ids_b; g.ldh = ld_ids_h; g.n = (int)n; g.T = (int)T; g.dist = dist;
  const dim3 grid((unsigned)(B * (n * (n + 1) / 2)));
  ED_BY_ROUTE(edit_route(T, T), R, hipLaunchKernelGGL(nbest_pairwise_kernel<R>, grid, dim3(64), sizeof(int64_t) * (size_t)T, (hipStream_t)stream, g));
  FK_CHECK_LAUNCH("fk_nbest_pairwise_distance");
  return FK_OK;
}

int fk_mbr_rank(const int32_t* dist, const float* scores, float scale, const int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, const int64_t* lengths,
                int64_t B, int64_t n, int64_t T, int64_t pad, float* risk, int64_t* ids_out, int64_t* lengths_out, float* scores_out, float* risk_out,
                int64_t* order, int64_t* n_valid, void* stream) {
  FK_CHECK_ARG(dist && scores && ids && lengths, "fk_mbr_rank: null pointer (input)");
  FK_CHECK_ARG(risk && ids_out && lengths_out && scores_out && risk_out && order && n_valid, "fk_mbr_rank: null pointer (output)");
  FK_CHECK_ARG(isfinite(scale), "fk_mbr_rank: scale is not finite");
  FK_CHECK_ARG(n >= 1 && n <= FK_NBEST_MAX_HYPS, "fk_mbr_rank: n = %lld hypotheses outside the envelope (1 .. %d)", (long long)n, FK_NBEST_MAX_HYPS);
  FK_CHECK_ARG(T >= 1 && T <= FK_NBEST_MAX_T, "fk_mbr_rank: T = %lld outside the envelope (1 .. %d)", (long long)T, FK_NBEST_MAX_T);
  FK_CHECK_ARG(B > 0 && B < (1LL << 31), "fk_mbr_rank: B = %lld", (long long)B);
  FK_CHECK_ARG(ld_ids_h >= T && ld_ids_b >= (n - 1) * ld_ids_h + T, "fk_mbr_rank: ids strides %lld / %lld below [n = %lld, T = %lld]",
               (long long)ld_ids_b, (long long)ld_ids_h, (long long)n, (long long)T);
  MbrArgs g;
  g.dist = dist; g.scores = scores; g.scale = scale; g.ids = ids; g.ldb = ld_ids_b; g.ldh = ld_ids_h; g.lengths = lengths; g.n = (int)n; g.T = (int)T;
  g.pad = pad; g.risk = risk; g.ids_out = ids_out; g.len_out = lengths_out; g.scores_out = scores_out; g.risk_out = risk_out; g.order = order;
  g.n_valid = n_valid;
  hipLaunchKernelGGL(mbr_rank_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, g);
  FK_CHECK_LAUNCH("fk_mbr_rank");
  return FK_OK;
}

int fk_mwer_combine(const float* nll, const int32_t* errors, const float* scores, const int64_t* lengths, int64_t max_len, int64_t B, int64_t n,
                    float* loss, float* coef, float* count, uint8_t* valid, void* stream) {
  FK_CHECK_ARG(nll && errors && loss && coef && count, "fk_mwer_combine: null pointer");
  FK_CHECK_ARG(n >= 1 && n <= FK_NBEST_MAX_HYPS, "fk_mwer_combine: n = %lld hypotheses outside the envelope (1 .. %d)", (long long)n, FK_NBEST_MAX_HYPS);
  FK_CHECK_ARG(B > 0 && B < (1LL << 24), "fk_mwer_combine: B = %lld", (long long)B);
  MwerArgs g;
  g.nll = nll; g.errors = errors; g.scores = scores; g.lengths = lengths; g.max_len = max_len; g.B = (int)B; g.n = (int)n;
  g.loss = loss; g.coef = coef; g.count = count; g.valid = valid;
  hipLaunchKernelGGL(mwer_combine_kernel, dim3(1), dim3(MW_THREADS), 0, (hipStream_t)stream, g);
  FK_CHECK_LAUNCH("fk_mwer_combine");
  return FK_OK;
}

int fk_mwer_reduce_rows(const void* rows, const uint8_t* valid, void* out, int64_t B, int64_t n, int64_t row_elems, int accumulate, int dtype,
                        void* stream) {
  FK_DT_CHECK("fk_mwer_reduce_rows");
  FK_CHECK_ARG(rows && valid && out, "fk_mwer_reduce_rows: null pointer");
  FK_CHECK_ARG(n >= 1 && n <= FK_NBEST_MAX_HYPS, "fk_mwer_reduce_rows: n = %lld hypotheses outside the envelope (1 .. %d)", (long long)n, FK_NBEST_MAX_HYPS);
  FK_CHECK_ARG(B > 0 && B < (1LL << 24) && row_elems > 0, "fk_mwer_reduce_rows: B = %lld, row_elems = %lld", (long long)B, (long long)row_elems);
  FK_BY_DTYPE(dtype, T, hipLaunchKernelGGL(mwer_reduce_rows_kernel<T>, dim3(fk_grid(B * row_elems, 16384)), dim3(FK_TPB), 0, (hipStream_t)stream,
                                           (const T*)rows, valid, (T*)out, (int)B, (int)n, row_elems, accumulate));
  FK_CHECK_LAUNCH("fk_mwer_reduce_rows");
  return FK_OK;
}
