// rescore.hip — language-model rescoring of an n-best list (the CTC prefix beam search's, csrc/ctc.hip) with the hypotheses of a sentence
// packed as a TRIE: every distinct token prefix is one row of one GPT forward under an ancestor mask, the vocabulary head runs through
// fk_head_ce_fwd (no [rows, V] logits), and the per-hypothesis sums, the combination with the acoustic score and the ranking stay on the
// device.  Semantics: include/franken_hip.h ("n-best rescoring"); tests/rescore_ref.py restates them in float64.
//
//   fk_nbest_trie       one workgroup per sentence: the hypotheses are inserted in order; the longest common prefix of hypothesis h with
//                       the earlier inserted ones says which of its positions already have a node, so the new nodes are the consecutive
//                       numbers behind it (no hash table, no global atomics).  A hypothesis is remembered as (L, g, base): its first L
//                       positions are those of hypothesis g, position j >= L is node base + j - L.
//   fk_nbest_trie_mask  one workgroup per row of the [P + N, P + N] visibility table
//   fk_gpt_embed_pos    the GPT input embedding with a position per row
//   fk_nbest_rescore    one workgroup per sentence: log-probabilities of the head rows, sums along the trie level by level (the adds of
//                       the sequential rule, in its order), totals, ranking by counting, gather into the new order
#include "fk_common.h"

#include <math.h>

namespace {

constexpr int NB_MAX = FK_NBEST_MAX_HYPS;
constexpr int NB_THREADS = 256;

struct TrieArgs {
  const int64_t* ids; int64_t ldb, ldh; const int64_t* lengths; const float* am;
  int n, T, cap, P; int64_t V, bos, eos;
  int *tok, *depth, *parent, *leaf, *n_nodes; int64_t *head_src, *head_tgt;
};

// node of position j of the inserted hypothesis h (j below its length): walk to the hypothesis that created it
FK_DEV int nb_node(const int* sL, const int* sg, const int* sbase, int h, int j) {
  while (j < sL[h]) h = sg[h];
  return sbase[h] + (j - sL[h]);
}

__global__ __launch_bounds__(NB_THREADS) void nbest_trie_kernel(TrieArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n, cap = a.cap;
  __shared__ int s_len[NB_MAX], s_L[NB_MAX], s_g[NB_MAX], s_base[NB_MAX], s_ins[NB_MAX], s_lcp[NB_MAX], s_leaf[NB_MAX];
  __shared__ int s_bad, s_nn, s_fp, s_new, s_Lc;
  const int64_t* ids = a.ids + (int64_t)b * a.ldb;
  int* tok = a.tok + (int64_t)b * cap;
  int* depth = a.depth + (int64_t)b * cap;
  int* parent = a.parent + (int64_t)b * cap;
  if (tid < n) {
    int64_t l = a.lengths[(int64_t)b * n + tid];
    s_len[tid] = (int)(l < 0 ? 0 : (l > a.T ? a.T : l));
    s_ins[tid] = 0;
  }
  if (tid == 0) {
    s_nn = 1;
    tok[0] = (int)a.bos; depth[0] = 0; parent[0] = -1;
  }
  for (int h = 0; h < n; ++h) {
    __syncthreads();                                                    // the last round's reads of s_bad / s_new are done
    const int len = s_len[h];
    const int64_t* x = ids + (int64_t)h * a.ldh;
    if (tid == 0) s_bad = (a.am && !isfinite(a.am[(int64_t)b * n + h])) ? 1 : 0;
    if (tid < h) s_lcp[tid] = len < s_len[tid] ? len : s_len[tid];
    __syncthreads();
    for (int j = tid; j < len; j += NB_THREADS) {
      const int64_t t = x[j];
      if (t < 0 || t >= a.V) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {                                                        // uniform: read behind a barrier
      if (tid == 0) { a.leaf[(int64_t)b * n + h] = -1; s_leaf[h] = -1; }
      continue;
    }
    for (int idx = tid; idx < h * len; idx += NB_THREADS) {             // first position at which h leaves each earlier hypothesis
      const int g = idx / len, j = idx - g * len;
      if (s_ins[g] && j < s_len[g] && ids[(int64_t)g * a.ldh + j] != x[j]) atomicMin(&s_lcp[g], j);
    }
    __syncthreads();
    if (tid == 0) {
      int L = 0, gs = -1;
      for (int g = 0; g < h; ++g)
        if (s_ins[g] && (gs < 0 || s_lcp[g] > L)) { L = s_lcp[g]; gs = g; }
      const int nw = len - L;
      int lf = -1, made = 0;
      if (s_nn + nw <= cap) {                                           // the overflow rule: all new nodes fit, or none is made
        s_L[h] = L; s_g[h] = gs < 0 ? 0 : gs; s_base[h] = s_nn; s_ins[h] = 1;
        s_fp = L == 0 ? 0 : nb_node(s_L, s_g, s_base, gs, L - 1);
        s_nn += nw;
        made = nw;
        lf = len == 0 ? 0 : nb_node(s_L, s_g, s_base, h, len - 1);
      }
      s_new = made; s_Lc = L;
      a.leaf[(int64_t)b * n + h] = lf; s_leaf[h] = lf;
    }
    __syncthreads();
    const int nw = s_new, L = s_Lc, base = s_base[h], fp = s_fp;
    for (int k = tid; k < nw; k += NB_THREADS) {
      const int i = base + k;
      tok[i] = (int)x[L + k]; depth[i] = L + k + 1; parent[i] = k == 0 ? fp : i - 1;
    }
  }
  __threadfence_block();
  __syncthreads();
  const int nn = s_nn;
  if (tid == 0) a.n_nodes[b] = nn;
  for (int i = nn + tid; i < cap; i += NB_THREADS) { tok[i] = (int)a.bos; depth[i] = 0; parent[i] = -1; }     // dead nodes
  if (a.head_src) {
    int64_t* src = a.head_src + (int64_t)b * (cap - 1 + n);
    int64_t* tgt = a.head_tgt + (int64_t)b * (cap - 1 + n);
    for (int i = 1 + tid; i < cap; i += NB_THREADS) {
      const bool live = i < nn;
      src[i - 1] = a.P + (live ? parent[i] : 0);
      tgt[i - 1] = live ? tok[i] : -100;
    }
    if (tid < n) {
      const int lf = s_leaf[tid];
      src[cap - 1 + tid] = a.P + (lf < 0 ? 0 : lf);
      tgt[cap - 1 + tid] = (a.eos >= 0 && lf >= 0) ? a.eos : -100;
    }
  }
}

__global__ __launch_bounds__(NB_THREADS) void nbest_mask_kernel(const int* parent, const int* n_nodes, uint8_t* mask, int P, int N) {
  const int q = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, R = P + N;
  __shared__ uint8_t s_anc[FK_NBEST_MAX_ROWS];
  uint8_t* row = mask + ((int64_t)b * R + q) * R;
  if (q < P) {
    for (int k = tid; k < R; k += NB_THREADS) row[k] = k <= q ? 1 : 0;
    return;
  }
  const int i = q - P;
  if (i >= n_nodes[b]) {                                                // a dead node sees itself
    for (int k = tid; k < R; k += NB_THREADS) row[k] = k == q ? 1 : 0;
    return;
  }
  for (int k = tid; k < N; k += NB_THREADS) s_anc[k] = 0;
  __syncthreads();
  if (tid == 0) {
    const int* par = parent + (int64_t)b * N;
    int a = i;
    while (a >= 0) {                                                    // parent[a] < a: at most i + 1 steps, all inside [0, i]
      s_anc[a] = 1;
      const int p = par[a];
      if (p >= a) break;
      a = p;
    }
  }
  __syncthreads();
  for (int k = tid; k < R; k += NB_THREADS) row[k] = k < P ? 1 : s_anc[k - P];
}

template <typename T>
__global__ void gpt_embed_pos_kernel(const int* tok, const int* depth, const T* prefix, const float* wte, const float* wpe, T* out, int B, int P,
                                     int N, int dim, int vocab, int wpe_rows) {
  const int R = P + N;
  const int64_t total = (int64_t)B * R * dim;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % dim);
    const int64_t row = i / dim;
    const int t = (int)(row % R), b = (int)(row / R);
    float v;
    int pos;
    if (t < P) {
      v = to_f32<T>(prefix[((int64_t)b * P + t) * dim + c]);
      pos = t;
    } else {
      int id = tok[(int64_t)b * N + (t - P)];
      id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
      v = wte[(int64_t)id * dim + c];
      int d = depth[(int64_t)b * N + (t - P)];
      pos = P + (d < 0 ? 0 : d);
    }
    pos = pos >= wpe_rows ? wpe_rows - 1 : pos;
    out[i] = from_f32<T>(v + wpe[(int64_t)pos * dim + c]);
  }
}

struct RescoreArgs {
  const float *row_m, *row_s, *row_t; const int *depth, *parent, *leaf, *n_nodes;
  const int64_t* ids; int64_t ldb, ldh; const int64_t* lengths; const float* am;
  int n, T, N, has_eos; int64_t pad; float am_w, lm_w, len_b;
  float* lm_in; int64_t* ids_out; int64_t* len_out; float *am_out, *lm_out, *total_out; int64_t *order, *n_scored;
};

__global__ __launch_bounds__(NB_THREADS) void nbest_rescore_kernel(RescoreArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n, N = a.N, Rh = N - 1 + n;
  __shared__ float s_cum[FK_NBEST_MAX_ROWS];
  __shared__ float s_tot[NB_MAX], s_lm[NB_MAX], s_am[NB_MAX];
  __shared__ int s_sc[NB_MAX], s_len[NB_MAX], s_rank[NB_MAX], s_maxd;
  const float* rm = a.row_m + (int64_t)b * Rh;
  const float* rs = a.row_s + (int64_t)b * Rh;
  const float* rt = a.row_t + (int64_t)b * Rh;
  const int* depth = a.depth + (int64_t)b * N;
  const int* parent = a.parent + (int64_t)b * N;
  int nn = a.n_nodes[b];
  nn = nn < 1 ? 1 : (nn > N ? N : nn);
  if (tid == 0) { s_maxd = 0; s_cum[0] = 0.0f; }
  __syncthreads();
  for (int i = 1 + tid; i < nn; i += NB_THREADS) atomicMax(&s_maxd, depth[i]);
  __syncthreads();
  const int maxd = s_maxd > a.T ? a.T : s_maxd;
  for (int d = 1; d <= maxd; ++d) {                                     // cum[i] = cum[parent[i]] + lp[i - 1]: a level reads only the one above
    for (int i = 1 + tid; i < nn; i += NB_THREADS)
      if (depth[i] == d) {
        int p = parent[i];
        p = (p < 0 || p >= i) ? 0 : p;
        s_cum[i] = s_cum[p] + (rt[i - 1] - (rm[i - 1] + logf(rs[i - 1])));
      }
    __syncthreads();
  }
  if (tid < n) {
    const int h = tid;
    const int lf = a.leaf[(int64_t)b * n + h];
    int64_t l = a.lengths[(int64_t)b * n + h];
    const int len = (int)(l < 0 ? 0 : (l > a.T ? a.T : l));
    const float amv = a.am ? a.am[(int64_t)b * n + h] : 0.0f;
    const bool scored = lf >= 0 && lf < nn;
    float lm = -INFINITY, tot = -INFINITY;
    if (scored) {
      lm = s_cum[lf];
      if (a.has_eos) lm += rt[N - 1 + h] - (rm[N - 1 + h] + logf(rs[N - 1 + h]));
      tot = a.am_w * amv + a.lm_w * lm + a.len_b * (float)len;
    }
    s_tot[h] = tot; s_lm[h] = lm; s_am[h] = amv; s_sc[h] = scored ? 1 : 0; s_len[h] = len;
    a.lm_in[(int64_t)b * n + h] = lm;
  }
  __syncthreads();
  if (tid < n) {
    const int h = tid;
    int rank = 0, cnt = 0;
    for (int g = 0; g < n; ++g) {
      cnt += s_sc[g];
      if (g == h) continue;
      bool beats;
      if (s_sc[g] != s_sc[h]) beats = s_sc[g] != 0;
      else if (!s_sc[g]) beats = g < h;
      else beats = s_tot[g] > s_tot[h] || (!(s_tot[h] > s_tot[g]) && g < h);
      rank += beats ? 1 : 0;
    }
    s_rank[h] = rank;
    const int64_t o = (int64_t)b * n + rank;
    a.len_out[o] = s_len[h]; a.am_out[o] = s_am[h]; a.lm_out[o] = s_lm[h]; a.total_out[o] = s_tot[h]; a.order[o] = h;
    if (h == 0) a.n_scored[b] = cnt;
  }
  __syncthreads();
  const int64_t* ids = a.ids + (int64_t)b * a.ldb;
  int64_t* out = a.ids_out + (int64_t)b * n * a.T;
  for (int idx = tid; idx < n * a.T; idx += NB_THREADS) {
    const int h = idx / a.T, j = idx - h * a.T;
    out[(int64_t)s_rank[h] * a.T + j] = j < s_len[h] ? ids[(int64_t)h * a.ldh + j] : a.pad;
  }
}

}  // namespace

int fk_nbest_trie(const int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, const int64_t* lengths, const float* am, int64_t B, int64_t n, int64_t T,
                  int64_t V, int64_t bos, int64_t eos, int64_t node_cap, int64_t P, int32_t* tok, int32_t* depth, int32_t* parent, int32_t* leaf,
                  int32_t* n_nodes, int64_t* head_src, int64_t* head_tgt, void* stream) {
  FK_CHECK_ARG(ids && lengths && tok && depth && parent && leaf && n_nodes, "fk_nbest_trie: null pointer");
  FK_CHECK_ARG((head_src == nullptr) == (head_tgt == nullptr), "fk_nbest_trie: head_src and head_tgt come together");
  FK_CHECK_ARG(B > 0 && B < (1LL << 31), "fk_nbest_trie: B = %lld", (long long)B);
  FK_CHECK_ARG(n >= 1 && n <= FK_NBEST_MAX_HYPS, "fk_nbest_trie: n = %lld hypotheses outside the envelope (1 .. %d)", (long long)n, FK_NBEST_MAX_HYPS);
  FK_CHECK_ARG(T >= 1 && T <= FK_NBEST_MAX_T, "fk_nbest_trie: T = %lld outside the envelope (1 .. %d)", (long long)T, FK_NBEST_MAX_T);
  FK_CHECK_ARG(node_cap >= 1 && node_cap <= FK_NBEST_MAX_NODES, "fk_nbest_trie: node_cap = %lld outside the envelope (1 .. %d)", (long long)node_cap,
               FK_NBEST_MAX_NODES);
  FK_CHECK_ARG(V >= 1 && V < (1LL << 31) && bos >= 0 && bos < V && eos >= -1 && eos < V, "fk_nbest_trie: V = %lld, bos = %lld, eos = %lld (-1: none)",
               (long long)V, (long long)bos, (long long)eos);
  FK_CHECK_ARG(P >= 0 && P < (1LL << 30), "fk_nbest_trie: P = %lld", (long long)P);
  FK_CHECK_ARG(ld_ids_h >= T && ld_ids_b >= (n - 1) * ld_ids_h + T, "fk_nbest_trie: ids strides %lld / %lld below [n = %lld, T = %lld]",
               (long long)ld_ids_b, (long long)ld_ids_h, (long long)n, (long long)T);
  TrieArgs a;
  a.ids = ids; a.ldb = ld_ids_b; a.ldh = ld_ids_h; a.lengths = lengths; a.am = am; a.n = (int)n; a.T = (int)T; a.cap = (int)node_cap; a.P = (int)P;
  a.V = V; a.bos = bos; a.eos = eos; a.tok = tok; a.depth = depth; a.parent = parent; a.leaf = leaf; a.n_nodes = n_nodes;
  a.head_src = head_src; a.head_tgt = head_tgt;
  hipLaunchKernelGGL(nbest_trie_kernel, dim3((unsigned)B), dim3(NB_THREADS), 0, (hipStream_t)stream, a);
  FK_CHECK_LAUNCH("fk_nbest_trie");
  return FK_OK;
}

int fk_nbest_trie_mask(const int32_t* parent, const int32_t* n_nodes, uint8_t* mask, int64_t B, int64_t P, int64_t N, void* stream) {
  FK_CHECK_ARG(parent && n_nodes && mask, "fk_nbest_trie_mask: null pointer");
  FK_CHECK_ARG(B > 0 && B < 65536, "fk_nbest_trie_mask: B = %lld", (long long)B);
  FK_CHECK_ARG(P >= 0 && N >= 1 && P + N <= FK_NBEST_MAX_ROWS, "fk_nbest_trie_mask: P = %lld, N = %lld outside the envelope (N >= 1, P + N <= %d)",
               (long long)P, (long long)N, FK_NBEST_MAX_ROWS);
  hipLaunchKernelGGL(nbest_mask_kernel, dim3((unsigned)(P + N), (unsigned)B), dim3(NB_THREADS), 0, (hipStream_t)stream, parent, n_nodes, mask, (int)P,
                     (int)N);
  FK_CHECK_LAUNCH("fk_nbest_trie_mask");
  return FK_OK;
}

int fk_gpt_embed_pos(const int32_t* tok, const int32_t* depth, const void* prefix, const float* wte, const float* wpe, void* out, int64_t B, int64_t P,
                     int64_t N, int64_t dim, int64_t vocab, int64_t wpe_rows, int dtype, void* stream) {
  FK_DT_CHECK("fk_gpt_embed_pos");
  FK_CHECK_ARG(tok && depth && wte && wpe && out, "fk_gpt_embed_pos: null pointer");
  FK_CHECK_ARG(P == 0 || prefix, "fk_gpt_embed_pos: prefix is NULL but P > 0");
  FK_CHECK_ARG(B > 0 && P >= 0 && N >= 1 && dim > 0 && vocab > 0 && vocab < (1LL << 31) && wpe_rows > P && B * (P + N) < (1LL << 31),
               "fk_gpt_embed_pos: B = %lld, P = %lld, N = %lld, dim = %lld, vocab = %lld, wpe_rows = %lld", (long long)B, (long long)P, (long long)N,
               (long long)dim, (long long)vocab, (long long)wpe_rows);
  const int64_t work = B * (P + N) * dim;
  FK_BY_DTYPE(dtype, T, hipLaunchKernelGGL(gpt_embed_pos_kernel<T>, dim3(fk_grid(work, 16384)), dim3(FK_TPB), 0, (hipStream_t)stream, tok, depth,
                                           (const T*)prefix, wte, wpe, (T*)out, (int)B, (int)P, (int)N, (int)dim, (int)vocab, (int)wpe_rows));
  FK_CHECK_LAUNCH("fk_gpt_embed_pos");
  return FK_OK;
}

int fk_nbest_rescore(const float* row_m, const float* row_s, const float* row_t, const int32_t* depth, const int32_t* parent, const int32_t* leaf,
                     const int32_t* n_nodes, const int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, const int64_t* lengths, const float* am, int64_t B,
                     int64_t n, int64_t T, int64_t N, int has_eos, float am_weight, float lm_weight, float length_bonus, int64_t pad, float* lm,
                     int64_t* ids_out, int64_t* lengths_out, float* am_out, float* lm_out, float* total_out, int64_t* order, int64_t* n_scored,
                     void* stream) {
  FK_CHECK_ARG(row_m && row_s && row_t && depth && parent && leaf && n_nodes && ids && lengths, "fk_nbest_rescore: null pointer (input)");
  FK_CHECK_ARG(lm && ids_out && lengths_out && am_out && lm_out && total_out && order && n_scored, "fk_nbest_rescore: null pointer (output)");
  FK_CHECK_ARG(B > 0 && B < (1LL << 31), "fk_nbest_rescore: B = %lld", (long long)B);
  FK_CHECK_ARG(n >= 1 && n <= FK_NBEST_MAX_HYPS, "fk_nbest_rescore: n = %lld hypotheses outside the envelope (1 .. %d)", (long long)n, FK_NBEST_MAX_HYPS);
  FK_CHECK_ARG(T >= 1 && T <= FK_NBEST_MAX_T, "fk_nbest_rescore: T = %lld outside the envelope (1 .. %d)", (long long)T, FK_NBEST_MAX_T);
  FK_CHECK_ARG(N >= 1 && N <= FK_NBEST_MAX_ROWS, "fk_nbest_rescore: N = %lld node rows outside the envelope (1 .. %d)", (long long)N, FK_NBEST_MAX_ROWS);
  FK_CHECK_ARG(ld_ids_h >= T && ld_ids_b >= (n - 1) * ld_ids_h + T, "fk_nbest_rescore: ids strides %lld / %lld below [n = %lld, T = %lld]",
               (long long)ld_ids_b, (long long)ld_ids_h, (long long)n, (long long)T);
  RescoreArgs a;
  a.row_m = row_m; a.row_s = row_s; a.row_t = row_t; a.depth = depth; a.parent = parent; a.leaf = leaf; a.n_nodes = n_nodes;
  a.ids = ids; a.ldb = ld_ids_b; a.ldh = ld_ids_h; a.lengths = lengths; a.am = am; a.n = (int)n; a.T = (int)T; a.N = (int)N; a.has_eos = has_eos != 0;
  a.pad = pad; a.am_w = am_weight; a.lm_w = lm_weight; a.len_b = length_bonus;
  a.lm_in = lm; a.ids_out = ids_out; a.len_out = lengths_out; a.am_out = am_out; a.lm_out = lm_out; a.total_out = total_out; a.order = order;
  a.n_scored = n_scored;
  hipLaunchKernelGGL(nbest_rescore_kernel, dim3((unsigned)B), dim3(NB_THREADS), 0, (hipStream_t)stream, a);
  FK_CHECK_LAUNCH("fk_nbest_rescore");
  return FK_OK;
}
