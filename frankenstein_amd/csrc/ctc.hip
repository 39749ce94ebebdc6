// ctc.hip — connectionist temporal classification: loss, gradient and greedy collapse for a frame-synchronous phoneme / token head.
//
// Semantics: F.ctc_loss(log_softmax(logits, -1).transpose(0, 1), targets, input_lengths, target_lengths, blank, reduction,
// zero_infinity) with the log-softmax folded in.  The reference project has no CTC; the yardstick is torch's float64 CPU loss.
//
//   fk_ctc_loss_fwd  launch 1  ctc_row_lse_kernel  row_lse[b, t] = logsumexp_c logits[b, t, c]; each logit is read once (online max / sum)
//                    launch 2  ctc_lattice_kernel  one workgroup per (sample, direction): alpha runs forward in time, beta backward, side by
//                              side; thread s owns extended state s of l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1
//                                wave route (2 Lmax + 1 <= 64):  one wave, the state vector in registers, neighbours by cross-lane moves,
//                                                                no LDS access and no barrier in the time loop
//                                LDS route  (2 Lmax + 1 <= 511): up to 512 threads, the state vector double-buffered in LDS, one barrier a step
//                              the operands logits[b, t, l'_s] - row_lse[b, t] of the next CTC_PF steps are in flight while a step computes
//                    launch 3  ctc_final_kernel    loss2 = {reduced loss, B} (one workgroup, fixed order)
//   fk_ctc_loss_bwd  one launch, row-parallel over [B T, C]:
//                      dlogits[b,t,c] = g_b (exp(logit - lse) - exp(logsumexp_{s: l'_s = c}(alpha_t(s) + beta_t(s)) + nll_b - (logit - lse)))
//                    the softmax term is a vector sweep of the row; the states of one class are summed in a fixed order (blank states: a
//                    tree; a label: its first occurrence walks the chain of later occurrences that the forward recorded) — no atomics.
//   fk_ctc_align     forced alignment (semantics: include/franken_hip.h; float64 restatement tests/ctc_align_ref.py)
//                    launch 1  ctc_row_lse_kernel  as above
//                    launch 2  ctc_align_kernel    one workgroup per sample on the lattice kernel's two routes: the alpha sweep with max for
//                              logsumexp and a 2-bit back-pointer per (t, s), sixteen frames a dword; then the same workgroup walks back in
//                              chunks of 256 frames whose back-pointers sit in LDS, and writes path, index, spans and per-label sums
//   fk_ctc_collapse  greedy decoding behind fk_argmax_rows: merge repeated frames, drop blanks, ordered compaction by ballot + prefix count
//   fk_ctc_beam_search  prefix beam search, n-best with scores (semantics: include/franken_hip.h; float64 restatement tests/ctc_beam_ref.py)
//                    launch 1  ctc_beam_prune_kernel  row-parallel like row_lse: one sweep of the row gives row_lse, lp[blank] and the K best
//                              non-blank (lp, id); a wave appends what beats its K-th best so far to an LDS buffer and compacts it when full
//                    launch 2  ctc_beam_kernel        one workgroup per sample, sequential over the frames: beam state in LDS, prefixes as a
//                              trie in the workspace, the W best of at most W + W K keys (in registers) by two rank counts
//   fk_ctc_beam_search_lm  the same search with a backoff n-gram model inside the selection (shallow fusion; float64 restatement
//                    tests/ctc_lm_ref.py): launch 1 as above, launch 2 the LM instantiation of ctc_beam_kernel, whose slots also carry the
//                    LM term, the LM sum and the LM state of their prefix (in LDS); the model is a state machine over one hash table
//   fk_ctc_beam_search_lex  the same search constrained to the words of a pronunciation lexicon, a word-level n-gram model at word ends
//                    (float64 restatement tests/ctc_lex_ref.py): launch 1 as above, launch 2 the lexicon instantiation of ctc_beam_kernel,
//                    whose slots also carry the trie node of their unfinished word and their word count; the trie is a hash table of edges
//
//   fk_ctc_prefix_init / fk_ctc_prefix_score  CTC prefix scores for the candidates of the GPT beam search (joint CTC / attention decoding;
//                    semantics: include/franken_hip.h; float64 restatement tests/ctc_prefix_ref.py): launch 1 of init as above, then one
//                    wave per sentence / per beam row: the hypothesis' state r_n / r_b [T] in LDS, the k candidates on the lanes
//
// row_lse, the backward and the prune kernel share one row frame (RowFrame) and one launch (CTC_LAUNCH_ROWS: the route and the grid).
// Device-side clamps (every access stays inside the buffers whatever the integers say): input_length into [0, T], target_length into
// [0, Lmax] (clamp_len), a label into [0, C) and off the blank (a label equal to the blank becomes blank - 1, or 1 when the blank is
// 0).  With a clamped label the loss is meaningless but defined.
#include <math.h>

#include "fk_common.h"

namespace {

constexpr int CTC_PF = 8;            // time steps whose operands are loaded ahead of the recursion
constexpr int CTC_MAX_S = 511;       // 2 Lmax + 1 at the top of the envelope
constexpr int CTC_MAX_THREADS = 512;

static inline int ctc_spad(int64_t Lmax) { return (int)(((2 * Lmax + 1) + 63) / 64 * 64); }
static inline size_t a256(size_t n) { return (n + 255) & ~(size_t)255; }

// the workspace: per-sample records first (all a loss without gradient needs), then the two lattices
struct CtcWs {
  float* nll_raw;   // [B]        the loss before zero_infinity
  int* len;         // [B][2]     clamped {T_b, L_b}
  int* lab;         // [B][S_pad] class of extended state s (clamped)
  int* nxt;         // [B][S_pad] next state with the same label, -1 at the end of the chain
  int* first;       // [B][S_pad] 1 when no earlier state carries this label
  float* alpha;     // [B][T][S_pad]
  float* beta;      // [B][T][S_pad]
};
static inline size_t ctc_ws_carve(CtcWs& w, void* base, int64_t B, int64_t T, int S_pad) {
  char* p = (char*)base;
  size_t o = 0;
  w.nll_raw = (float*)(p + o); o += a256((size_t)B * sizeof(float));
  w.len = (int*)(p + o);       o += a256((size_t)B * 2 * sizeof(int));
  w.lab = (int*)(p + o);       o += a256((size_t)B * S_pad * sizeof(int));
  w.nxt = (int*)(p + o);       o += a256((size_t)B * S_pad * sizeof(int));
  w.first = (int*)(p + o);     o += a256((size_t)B * S_pad * sizeof(int));
  w.alpha = (float*)(p + o);   o += a256((size_t)B * T * S_pad * sizeof(float));
  w.beta = (float*)(p + o);    o += a256((size_t)B * T * S_pad * sizeof(float));
  return o;
}

// ---- group reductions: the group is one wave (shuffles only) or the whole workgroup (through sh, >= 8 floats; barriers) ---------------
template <typename V, typename Op> FK_DEV V across_waves(V v, V* sh, V init, Op op) {   // the waves' values folded in wave order from `init`
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = init;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) v = op(v, sh[i]);
  return v;
}
template <bool BLOCK> FK_DEV float group_max(float v, float* sh) {
  v = wave_max(v);
  if constexpr (BLOCK) v = across_waves(v, sh, -INFINITY, [](float a, float b) { return fmaxf(a, b); });
  return v;
}
template <bool BLOCK> FK_DEV float group_sum(float v, float* sh) {
  v = wave_sum(v);
  if constexpr (BLOCK) v = across_waves(v, sh, 0.0f, [](float a, float b) { return a + b; });
  return v;
}
FK_DEV int block_min_int(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return across_waves(v, sh, v, [](int a, int b) { return min(a, b); });
}

// input_lengths[b] into [0, T], target_lengths[b] into [0, Lmax]; no array: the full length
FK_DEV int clamp_len(const int64_t* lengths, int b, int hi) {
  if (!lengths) return hi;
  const int64_t v = lengths[b];
  return v < 0 ? 0 : (v > hi ? hi : (int)v);
}

// The frame of a one-workgroup-per-sample kernel over the extended states (the lattice, the alignment): thread s owns state s of
// l' = (blank, l_1, blank, ..., l_L, blank).
// L_b: target_lengths[b] clamped, or without the array the leading entries of the row tg that differ from pad_value (every thread of the
// workgroup calls it; sh: 8 ints; it holds barriers)
FK_DEV int target_len(const int64_t* target_lengths, const int64_t* tg, int64_t pad_value, int b, int Lmax, int* sh) {
  if (target_lengths) return clamp_len(target_lengths, b, Lmax);
  int f = Lmax;
  for (int i = threadIdx.x; i < Lmax; i += blockDim.x)
    if (tg[i] == pad_value) { f = i; break; }
  return block_min_int(f, sh);
}
// the class of extended state s: a label clamped into [0, C) and off the blank, the blank for an even state or one behind the target
FK_DEV int state_label(const int64_t* tg, int s, int Lb, int C, int blank) {
  if (!(s & 1) || (s >> 1) >= Lb) return blank;
  int64_t l = tg[s >> 1];
  l = l < 0 ? 0 : (l >= C ? C - 1 : l);
  if (l == blank) l = blank == 0 ? 1 : blank - 1;
  return (int)l;
}
// state s exchanges mass with state `far` = s -+ 2 across the blank between them: both carry labels, and different ones (sh_lab: the
// classes of all CTC_MAX_THREADS states)
FK_DEV bool may_skip(const int* sh_lab, int s, int far, int S, int lab) {
  return s < S && (s & 1) && far >= 1 && far < S && sh_lab[far >= 0 && far < CTC_MAX_THREADS ? far : s] != lab;
}

// running (max, sum of exponentials) per lane, rescaled once per vector; exp(-inf - -inf) is never formed; returns the vector's own maximum
template <int N> FK_DEV float lse_push(float& m, float& s, const float (&v)[N]) {
  float best = v[0];
#pragma unroll
  for (int e = 1; e < N; ++e) best = fmaxf(best, v[e]);
  const float vm = fmaxf(m, best);
  if (vm > -INFINITY) {
    float acc = s * __expf(m - vm);
#pragma unroll
    for (int e = 0; e < N; ++e) acc += __expf(v[e] - vm);
    s = acc;
    m = vm;
  }
  return best;
}
FK_DEV void lse_push(float& m, float& s, float x) { const float v[1] = {x}; lse_push(m, s, v); }

// The frame of a row-parallel kernel (row_lse, backward, beam prune).  A group of G threads owns a row: the whole workgroup (BLOCK: one
// row a pass), or one wave of the four (four rows a pass, wave `sub` the row base + sub, base from f.first in steps of f.step: a
// block-uniform trip count); thread gl takes every G-th element or vector of the row.  A row is swept on the shared vector I/O: scalar
// elements up to its first 16-byte boundary (head), nvec whole vectors, a scalar tail.  Any row stride and any C take the vector body (C =
// 50258 in fp32 leaves every other row 8 bytes off the boundary).  The sweeps stay with the kernels: prune loads ahead, the backward stores.
template <typename T, bool BLOCK> struct RowFrame {
  static constexpr int N = VecIO<T>::N, G = BLOCK ? 256 : 64, RPB = BLOCK ? 1 : 4;
  const int gl = BLOCK ? threadIdx.x : (threadIdx.x & 63), sub = BLOCK ? 0 : (threadIdx.x >> 6);
  const int64_t first = (int64_t)blockIdx.x * RPB, step = (int64_t)gridDim.x * RPB;
  FK_DEV static int row_head(const T* p, int C) {       // elements in front of the first 16-byte boundary of the row at p, at most C
    const int h = (int)((N - (int)(((uintptr_t)p / sizeof(T)) % N)) % N);
    return h < C ? h : C;
  }
  struct Split { int head, nvec, tail; };               // [0, head) scalar, nvec vectors from head, [tail, C) scalar
  FK_DEV static Split split(int head, int C) { return {head, (C - head) / N, head + (C - head) / N * N}; }
  // the row's logsumexp from the lanes' (m, s); every thread of the workgroup calls it (sh: 8 floats; under BLOCK it holds barriers)
  FK_DEV static float finish(float m, float s, float* sh) {
    const float M = group_max<BLOCK>(m, sh);
    const float tot = group_sum<BLOCK>(m > -INFINITY ? s * __expf(m - M) : 0.0f, sh);
    return M + logf(tot);
  }
};

// ---- launch 1: row_lse -------------------------------------------------------------------------------------------------------
template <typename T, bool BLOCK>
__global__ __launch_bounds__(256) void ctc_row_lse_kernel(const T* logits, int64_t ldb, int64_t ldt, float* row_lse, int64_t rows, int T_, int C) {
  const RowFrame<T, BLOCK> f{};
  constexpr int N = f.N, G = f.G;
  __shared__ float sh[8];
  for (int64_t base = f.first; base < rows; base += f.step) {
    const int64_t row = base + f.sub;
    float m = -INFINITY, s = 0.0f;
    if (row < rows) {
      const T* lr = logits + (row / T_) * ldb + (row % T_) * ldt;
      const auto sp = f.split(f.row_head(lr, C), C);
      for (int c = f.gl; c < sp.head; c += G) lse_push(m, s, to_f32<T>(lr[c]));
      for (int i = f.gl; i < sp.nvec; i += G) {
        float v[N];
        VecIO<T>::load(lr + sp.head + i * N, v);
        lse_push(m, s, v);
      }
      for (int c = sp.tail + f.gl; c < C; c += G) lse_push(m, s, to_f32<T>(lr[c]));
    }
    const float lse = f.finish(m, s, sh);
    if (row < rows && f.gl == 0) row_lse[row] = lse;
  }
}

// ---- launch 2: the lattice -----------------------------------------------------------------------------------------------------
struct CtcFwdArgs {
  const void* logits;
  int64_t ldb, ldt;
  const int64_t* targets;
  int64_t ldtgt;
  const int64_t* input_lengths;
  const int64_t* target_lengths;
  int64_t pad_value;
  const float* row_lse;
  float* nll;
  CtcWs w;
  int T, C, Lmax, S_pad, blank, zero_inf, want_lattice;
};

// log(e^a + e^b + e^c); an all -inf triple gives -inf through log(0), never through inf - inf
FK_DEV float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  const float mm = m == -INFINITY ? 0.0f : m;
  return mm + __logf(__expf(a - mm) + __expf(b - mm) + __expf(c - mm));
}

template <typename T, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : CTC_MAX_THREADS) void ctc_lattice_kernel(CtcFwdArgs a) {
  constexpr int W = CTC_MAX_THREADS + 4;                // LDS route: state s at index s + 2, two -inf entries either side
  __shared__ int sh_lab[CTC_MAX_THREADS];
  __shared__ int sh_red[8];
  __shared__ float sh_fin[2];
  __shared__ float sh_st[WAVE ? 2 : 2 * W];
  const int b = blockIdx.x, dir = blockIdx.y, s = threadIdx.x;

  // lengths, clamped; without target_lengths: the leading entries that differ from pad_value
  const int Tb = clamp_len(a.input_lengths, b, a.T);
  const int64_t* tg = a.targets + (int64_t)b * a.ldtgt;
  const int Lb = target_len(a.target_lengths, tg, a.pad_value, b, a.Lmax, sh_red);
  const int S = 2 * Lb + 1;

  // the class of this thread's state
  const int lab = state_label(tg, s, Lb, a.C, a.blank);
  sh_lab[s] = lab;
  __syncthreads();
  const bool live = s < S, odd = (s & 1) != 0;

  if (dir == 0) {
    // what the backward needs beside the lattice: lengths, classes and, per label, the chain of its states in index order
    int first = 0, nxt = -1;
    if (a.want_lattice && live && odd) {
      first = 1;
      for (int j = s - 2; j >= 1; j -= 2)
        if (sh_lab[j] == lab) { first = 0; break; }
      for (int j = s + 2; j < S; j += 2)
        if (sh_lab[j] == lab) { nxt = j; break; }
    }
    if (a.want_lattice) {
      const size_t o = (size_t)b * a.S_pad + s;
      a.w.lab[o] = lab;
      a.w.nxt[o] = nxt;
      a.w.first[o] = first;
    }
    if (s == 0) { a.w.len[2 * b] = Tb; a.w.len[2 * b + 1] = Lb; }
  }

  if (Tb == 0) {                                        // no frame: only the empty target has an alignment
    if (dir == 0 && s == 0) {
      const float raw = Lb == 0 ? 0.0f : INFINITY;
      a.w.nll_raw[b] = raw;
      a.nll[b] = (a.zero_inf && raw == INFINITY) ? 0.0f : raw;
    }
    return;
  }

  // alpha (dir 0) looks at s - 1 and s - 2 and walks t = 0 .. T_b - 1; beta (dir 1) looks at s + 1 and s + 2 and walks down from T_b - 1
  const int d = dir ? 1 : -1;
  const int far = s + 2 * d;
  const bool skip = may_skip(sh_lab, s, far, S, lab);
  const bool init = live && (dir ? (s >= S - 2) : (s <= 1));
  const T* lg = (const T*)a.logits + (int64_t)b * a.ldb + lab;
  const float* lse = a.row_lse + (int64_t)b * a.T;
  float* out = (dir ? a.w.beta : a.w.alpha) + ((size_t)b * a.T) * a.S_pad + s;

  T ql[CTC_PF], nl[CTC_PF];                             // raw operands: the subtraction waits at the step that uses them
  float qe[CTC_PF], ne[CTC_PF];
#pragma unroll
  for (int i = 0; i < CTC_PF; ++i) {
    const int k = i < Tb ? i : Tb - 1, t = dir ? Tb - 1 - k : k;
    ql[i] = lg[(int64_t)t * a.ldt];
    qe[i] = lse[t];
  }
  if constexpr (!WAVE) {
    if (s < 2) {
      sh_st[s] = sh_st[W + s] = -INFINITY;
      sh_st[a.S_pad + 2 + s] = sh_st[W + a.S_pad + 2 + s] = -INFINITY;
    }
  }
  float v = -INFINITY;
  for (int k0 = 0; k0 < Tb; k0 += CTC_PF) {
#pragma unroll
    for (int i = 0; i < CTC_PF; ++i) {
      const int kk = k0 + CTC_PF + i, k = kk < Tb ? kk : Tb - 1, t = dir ? Tb - 1 - k : k;
      nl[i] = lg[(int64_t)t * a.ldt];
      ne[i] = lse[t];
    }
#pragma unroll
    for (int i = 0; i < CTC_PF; ++i) {
      const int k = k0 + i;
      if (k < Tb) {                                     // workgroup-uniform
        const float lp = to_f32<T>(ql[i]) - qe[i];
        if (k == 0) {
          v = init ? lp : -INFINITY;
        } else {
          float n1, n2;
          if constexpr (WAVE) {
            const int near = s + d;
            n1 = __shfl(v, near & 63, 64);
            n2 = __shfl(v, far & 63, 64);
            n1 = (near >= 0 && near < 64) ? n1 : -INFINITY;
          } else {
            const float* cur = sh_st + ((k - 1) & 1) * W + s + 2;
            n1 = cur[d];
            n2 = cur[2 * d];
          }
          n2 = skip ? n2 : -INFINITY;
          v = live ? lse3(v, n1, n2) + lp : -INFINITY;
        }
        if constexpr (!WAVE) {
          sh_st[(k & 1) * W + s + 2] = v;
          __syncthreads();
        }
        if (a.want_lattice) out[(size_t)(dir ? Tb - 1 - k : k) * a.S_pad] = v;
      }
    }
#pragma unroll
    for (int i = 0; i < CTC_PF; ++i) { ql[i] = nl[i]; qe[i] = ne[i]; }
  }

  if (dir == 0) {                                       // nll = -log(e^alpha(S-1) + e^alpha(S-2)) at the last frame
    if (s == S - 1) { sh_fin[0] = v; if (S < 2) sh_fin[1] = -INFINITY; }
    if (s == S - 2) sh_fin[1] = v;
    __syncthreads();
    if (s == 0) {
      const float raw = -lse3(sh_fin[0], sh_fin[1], -INFINITY);
      a.w.nll_raw[b] = raw;
      a.nll[b] = (a.zero_inf && raw == INFINITY) ? 0.0f : raw;
    }
  }
}

// ---- forced alignment: the lattice in the max-plus semiring with a back-pointer per (t, s), then the walk back ---------------------------
// forward  v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if may_skip) + lp_t(l'_s); the move 0 / 1 / 2 that won (exact ties: the smaller
//          move) is two bits; a thread gathers the codes of CTC_ALIGN_PACK frames in a register and stores one dword: bp[b][t / PACK][s]
// backward CTC_ALIGN_CHUNK frames at a time from the last to the first: thread s copies column s of the chunk's packed rows (what it wrote
//          itself) into LDS, thread 0 walks the chunk there (a dependent LDS read a frame, no global access) and leaves the state per
//          frame in LDS, then all threads turn states into path / index and mark the span boundaries of the labels (in LDS)
// last     thread i stores start / end of label i and sums lp_t(l_i) over its frames in ascending order.  No atomics.
constexpr int CTC_ALIGN_PACK = 16;                      // frames per back-pointer dword
constexpr int CTC_ALIGN_CHUNK = 256;                    // frames per backtrack chunk
constexpr int ALIGN_ROWS = CTC_ALIGN_CHUNK / CTC_ALIGN_PACK;
static_assert(CTC_ALIGN_PACK * 2 == 32 && CTC_ALIGN_CHUNK % CTC_ALIGN_PACK == 0 && CTC_PF <= CTC_ALIGN_PACK && CTC_ALIGN_PACK % CTC_PF == 0,
              "a dword of 2-bit codes; whole dwords a chunk");
static_assert(ALIGN_ROWS * CTC_MAX_THREADS * 4 + (CTC_ALIGN_CHUNK + 2) * 4 + CTC_MAX_THREADS * 4 + 2 * 256 * 4 + 64 <= 40 * 1024,
              "ctc_align_kernel: LDS budget (four workgroups of 512 threads a CU: all 32 waves)");

struct CtcAlignWs {
  float* row_lse;   // [B T]
  unsigned* bp;     // [B][ceil(T / PACK)][S_pad] sixteen 2-bit moves a dword, frame t in bits 2 (t % PACK)
};
static inline size_t align_ws_carve(CtcAlignWs& w, void* base, int64_t B, int64_t T, int S_pad) {
  char* p = (char*)base;
  size_t o = 0;
  w.row_lse = (float*)(p + o); o += a256((size_t)B * T * sizeof(float));
  w.bp = (unsigned*)(p + o);   o += a256((size_t)B * fk_cdiv(T, CTC_ALIGN_PACK) * S_pad * sizeof(unsigned));
  return o;
}

struct CtcAlignArgs {
  const void* logits;
  int64_t ldb, ldt;
  const int64_t* targets;
  int64_t ldtgt;
  const int64_t* input_lengths;
  const int64_t* target_lengths;
  int64_t pad_value, pad;
  CtcAlignWs w;
  float* score;
  int64_t* path;
  int64_t ld_path;
  int64_t* index;
  int64_t ld_index;
  int64_t* start;
  int64_t* end;
  float* label_lp;
  int64_t ld_lab;
  int T, C, Lmax, S_pad, blank;
};

// what a sample holds where there is nothing to say: frames [t0, T) of path / index, labels [l0, Lmax) of start / end / label_lp
FK_DEV void align_fill(const CtcAlignArgs& a, int b, int t0, int l0) {
  for (int t = t0 + threadIdx.x; t < a.T; t += blockDim.x) {
    a.path[(int64_t)b * a.ld_path + t] = a.pad;
    if (a.index) a.index[(int64_t)b * a.ld_index + t] = -1;
  }
  for (int i = l0 + threadIdx.x; i < a.Lmax; i += blockDim.x) {
    if (a.start) a.start[(int64_t)b * a.ld_lab + i] = -1;
    if (a.end) a.end[(int64_t)b * a.ld_lab + i] = -1;
    if (a.label_lp) a.label_lp[(int64_t)b * a.ld_lab + i] = 0.0f;
  }
}

template <typename T, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : CTC_MAX_THREADS) void ctc_align_kernel(CtcAlignArgs a) {
  constexpr int W = CTC_MAX_THREADS + 4;                // LDS route: state s at index s + 2, two -inf entries either side
  constexpr int SW = WAVE ? 64 : CTC_MAX_THREADS;       // row stride of the chunk's back-pointers in LDS
  __shared__ int sh_lab[CTC_MAX_THREADS];
  __shared__ int sh_red[8];
  __shared__ float sh_fin[2];
  __shared__ unsigned sh_bp[ALIGN_ROWS * SW];
  float* sh_st = reinterpret_cast<float*>(sh_bp);       // the forward's double-buffered state vector: over before the first chunk is copied in
  static_assert(WAVE || 2 * W <= ALIGN_ROWS * SW, "the state vector fits into the chunk buffer");
  __shared__ int sh_state[CTC_ALIGN_CHUNK + 2];       // [1 + i]: the state at frame c0 + i; [0] and [n + 1]: the frames either side, -1: none
  __shared__ int sh_start[256], sh_end[256];            // per label (Lmax <= 255)
  const int b = blockIdx.x, s = threadIdx.x;

  const int Tb = clamp_len(a.input_lengths, b, a.T);
  const int64_t* tg = a.targets + (int64_t)b * a.ldtgt;
  const int Lb = target_len(a.target_lengths, tg, a.pad_value, b, a.Lmax, sh_red);
  const int S = 2 * Lb + 1;
  const int lab = state_label(tg, s, Lb, a.C, a.blank);
  sh_lab[s] = lab;
  if (s < 256) sh_start[s] = sh_end[s] = -1;
  __syncthreads();
  const bool live = s < S;

  if (Tb == 0) {                                        // no frame: only the empty target has an alignment, the empty one
    if (s == 0) a.score[b] = Lb == 0 ? 0.0f : -INFINITY;
    align_fill(a, b, 0, 0);
    return;
  }

  // ---- forward: the lattice kernel's alpha sweep with max for lse3 ----
  const bool skip = may_skip(sh_lab, s, s - 2, S, lab);
  const bool init = live && s <= 1;
  const T* lg = (const T*)a.logits + (int64_t)b * a.ldb + lab;
  const float* lse = a.w.row_lse + (int64_t)b * a.T;
  const int NP = (a.T + CTC_ALIGN_PACK - 1) / CTC_ALIGN_PACK;
  unsigned* bp = a.w.bp + (size_t)b * NP * a.S_pad + s;  // this thread's column: blockDim.x == S_pad on both routes

  T ql[CTC_PF], nl[CTC_PF];
  float qe[CTC_PF], ne[CTC_PF];
#pragma unroll
  for (int i = 0; i < CTC_PF; ++i) {
    const int t = i < Tb ? i : Tb - 1;
    ql[i] = lg[(int64_t)t * a.ldt];
    qe[i] = lse[t];
  }
  if constexpr (!WAVE) {
    if (s < 2) {
      sh_st[s] = sh_st[W + s] = -INFINITY;
      sh_st[a.S_pad + 2 + s] = sh_st[W + a.S_pad + 2 + s] = -INFINITY;
    }
  }
  float v = -INFINITY;
  unsigned codes = 0u;
  for (int k0 = 0; k0 < Tb; k0 += CTC_PF) {
#pragma unroll
    for (int i = 0; i < CTC_PF; ++i) {
      const int kk = k0 + CTC_PF + i, t = kk < Tb ? kk : Tb - 1;
      nl[i] = lg[(int64_t)t * a.ldt];
      ne[i] = lse[t];
    }
#pragma unroll
    for (int i = 0; i < CTC_PF; ++i) {
      const int k = k0 + i;
      if (k < Tb) {                                     // workgroup-uniform
        const float lp = to_f32<T>(ql[i]) - qe[i];
        if (k == 0) {
          v = init ? lp : -INFINITY;
        } else {
          float n1, n2;
          if constexpr (WAVE) {
            n1 = __shfl(v, (s - 1) & 63, 64);
            n2 = __shfl(v, (s - 2) & 63, 64);
            n1 = s >= 1 ? n1 : -INFINITY;
          } else {
            const float* cur = sh_st + ((k - 1) & 1) * W + s + 2;
            n1 = cur[-1];
            n2 = cur[-2];
          }
          n2 = skip ? n2 : -INFINITY;
          float best = v;                               // exact ties: stay before s - 1 before s - 2
          unsigned code = 0u;
          if (n1 > best) { best = n1; code = 1u; }
          if (n2 > best) { best = n2; code = 2u; }
          v = live ? best + lp : -INFINITY;
          codes |= code << (2 * (k & (CTC_ALIGN_PACK - 1)));
        }
        if constexpr (!WAVE) {
          sh_st[(k & 1) * W + s + 2] = v;
          __syncthreads();
        }
        if ((k & (CTC_ALIGN_PACK - 1)) == CTC_ALIGN_PACK - 1 || k == Tb - 1) {
          bp[(size_t)(k / CTC_ALIGN_PACK) * a.S_pad] = codes;
          codes = 0u;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CTC_PF; ++i) { ql[i] = nl[i]; qe[i] = ne[i]; }
  }

  // ---- the end state: the better of S - 1 and S - 2, S - 1 on an exact tie ----
  if (s == S - 1) { sh_fin[0] = v; if (S < 2) sh_fin[1] = -INFINITY; }
  if (s == S - 2) sh_fin[1] = v;
  __syncthreads();
  const float e0 = sh_fin[0], e1 = sh_fin[1];
  const float sc = e1 > e0 ? e1 : e0;
  if (s == 0) a.score[b] = sc;
  if (sc == -INFINITY) {                                // no alignment (workgroup-uniform)
    align_fill(a, b, 0, 0);
    return;
  }
  align_fill(a, b, Tb, Lb);

  // ---- backward: chunk by chunk, the walk in LDS ----
  int cur = e1 > e0 ? S - 2 : S - 1;                    // thread 0's: the state at the frame the walk stands at
  int after = -1;                                       //             the state at the first frame behind the chunk
  int64_t* path = a.path + (int64_t)b * a.ld_path;
  int64_t* index = a.index ? a.index + (int64_t)b * a.ld_index : nullptr;
  for (int c0 = (Tb - 1) / CTC_ALIGN_CHUNK * CTC_ALIGN_CHUNK; c0 >= 0; c0 -= CTC_ALIGN_CHUNK) {
    const int n = Tb - c0 < CTC_ALIGN_CHUNK ? Tb - c0 : CTC_ALIGN_CHUNK;
    const int rows = (n + CTC_ALIGN_PACK - 1) / CTC_ALIGN_PACK;
    unsigned col[ALIGN_ROWS];
#pragma unroll
    for (int r = 0; r < ALIGN_ROWS; ++r) col[r] = r < rows ? bp[(size_t)(c0 / CTC_ALIGN_PACK + r) * a.S_pad] : 0u;
#pragma unroll
    for (int r = 0; r < ALIGN_ROWS; ++r) sh_bp[r * SW + s] = col[r];
    __syncthreads();
    if (s == 0) {
      sh_state[n + 1] = after;
      for (int i = n - 1; i >= 0; --i) {
        sh_state[i + 1] = cur;
        after = cur;
        const unsigned code = (sh_bp[(i / CTC_ALIGN_PACK) * SW + cur] >> (2 * (i & (CTC_ALIGN_PACK - 1)))) & 3u;
        if (c0 + i > 0) {
          cur -= (int)code;
          cur = cur < 0 ? 0 : (cur >= S ? S - 1 : cur);
        }
      }
      sh_state[0] = c0 > 0 ? cur : -1;
    }
    __syncthreads();
    for (int i = s; i < n; i += blockDim.x) {
      const int st = sh_state[i + 1], t = c0 + i;
      path[t] = sh_lab[st];
      if (index) index[t] = (st & 1) ? (st >> 1) : -1;
      if (st & 1) {
        if (sh_state[i] != st) sh_start[st >> 1] = t;
        if (sh_state[i + 2] != st) sh_end[st >> 1] = t + 1;
      }
    }
    __syncthreads();
  }

  // ---- per label: its span and the sum of its log-probabilities along it, one add a frame in ascending order ----
  if (s < Lb) {
    int t0 = sh_start[s], t1 = sh_end[s];
    if (a.start) a.start[(int64_t)b * a.ld_lab + s] = t0;
    if (a.end) a.end[(int64_t)b * a.ld_lab + s] = t1;
    if (a.label_lp) {
      t0 = t0 < 0 ? 0 : t0;
      t1 = t1 > Tb ? Tb : t1;
      const T* lr = (const T*)a.logits + (int64_t)b * a.ldb + sh_lab[2 * s + 1];
      float sum = 0.0f;
      for (int t = t0; t < t1; ++t) sum += to_f32<T>(lr[(int64_t)t * a.ldt]) - lse[t];
      a.label_lp[(int64_t)b * a.ld_lab + s] = sum;
    }
  }
}

// ---- launch 3: loss2 = {reduced loss, B}; mean is torch's: nll_b / max(L_b, 1) averaged over all B ----------------------------------
__global__ void ctc_final_kernel(const float* nll, const int* len, float* loss2, int B, int reduction) {
  __shared__ float sh[8];
  float s = 0.0f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int L = len[2 * b + 1];
    s += reduction == FK_CTC_MEAN ? nll[b] / (float)(L > 1 ? L : 1) : nll[b];
  }
  s = group_sum<true>(s, sh);
  if (threadIdx.x == 0) { loss2[0] = reduction == FK_CTC_MEAN ? s / (float)B : s; loss2[1] = (float)B; }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
struct CtcBwdArgs {
  const void* logits;
  int64_t ldb, ldt;
  const float* row_lse;
  const float* gout;
  void* dl;
  int64_t lddb, lddt;
  CtcWs w;
  int B, T, C, S_pad, blank, reduction, zero_inf;
};

template <typename T, bool BLOCK>
__global__ __launch_bounds__(256) void ctc_bwd_kernel(CtcBwdArgs a) {
  const RowFrame<T, BLOCK> f{};
  constexpr int N = f.N, G = f.G;
  __shared__ float sh[8];
  const int gl = f.gl;
  const int64_t rows = (int64_t)a.B * a.T;
  for (int64_t base = f.first; base < rows; base += f.step) {
    const int64_t row = base + f.sub;
    int b = 0, t = 0, Lb = 0;
    float g = 0.0f, raw = 0.0f, lse = 0.0f;
    const T* lr = nullptr;
    T* dr = nullptr;
    bool full = false;
    if (row < rows) {
      b = (int)(row / a.T);
      t = (int)(row % a.T);
      const int Tb = a.w.len[2 * b];
      Lb = a.w.len[2 * b + 1];
      raw = a.w.nll_raw[b];
      lse = a.row_lse[row];
      lr = (const T*)a.logits + b * a.ldb + t * a.ldt;
      dr = (T*)a.dl + b * a.lddb + t * a.lddt;
      g = a.reduction == FK_CTC_NONE ? a.gout[b] : a.gout[0];
      if (a.reduction == FK_CTC_MEAN) g /= (float)a.B * (float)(Lb > 1 ? Lb : 1);
      const bool infeasible = raw == INFINITY;
      full = t < Tb && !infeasible;
      // a frame past the sample's end is exactly zero; an infeasible sample is zero under zero_infinity and NaN without, as torch's
      const float fill = (t < Tb && infeasible && !a.zero_inf) ? NAN : 0.0f;
      const int hl = f.row_head(lr, a.C), hd = f.row_head(dr, a.C);
      const auto sp = f.split(hl == hd ? hl : a.C, a.C);             // rows that disagree about the boundary go element by element
      for (int c = gl; c < sp.head; c += G) dr[c] = from_f32<T>(full ? g * __expf(to_f32<T>(lr[c]) - lse) : fill);
      for (int i = gl; i < sp.nvec; i += G) {
        float v[N], o[N];
        if (full) VecIO<T>::load(lr + sp.head + i * N, v);
#pragma unroll
        for (int e = 0; e < N; ++e) o[e] = full ? g * __expf(v[e] - lse) : fill;
        VecIO<T>::store(dr + sp.head + i * N, o);
      }
      for (int c = sp.tail + gl; c < a.C; c += G) dr[c] = from_f32<T>(full ? g * __expf(to_f32<T>(lr[c]) - lse) : fill);
    }
    __syncthreads();                                    // the classes of the target are rewritten below, behind the sweep's stores
    if (BLOCK ? full : true) {                          // (block-uniform under BLOCK: the reductions inside hold barriers)
      const size_t lo = ((size_t)(full ? b : 0) * a.T + (full ? t : 0)) * a.S_pad;
      const float* al = a.w.alpha + lo;
      const float* be = a.w.beta + lo;
      // blank: the even states, a tree in a fixed order
      float mx = -INFINITY;
      if (full)
        for (int i = gl; i <= Lb; i += G) mx = fmaxf(mx, al[2 * i] + be[2 * i]);
      mx = group_max<BLOCK>(mx, sh);
      float sm = 0.0f;
      if (full && mx > -INFINITY)
        for (int i = gl; i <= Lb; i += G) sm += __expf(al[2 * i] + be[2 * i] - mx);
      sm = group_sum<BLOCK>(sm, sh);
      if (full && gl == 0) {
        const float lp = to_f32<T>(lr[a.blank]) - lse;
        const float occ = mx > -INFINITY ? __expf(mx + __logf(sm) + raw - lp) : 0.0f;
        dr[a.blank] = from_f32<T>(g * (__expf(lp) - occ));
      }
      // a label: its first state walks the chain of its later states serially
      if (full) {
        const int* lab = a.w.lab + (size_t)b * a.S_pad;
        const int* nxt = a.w.nxt + (size_t)b * a.S_pad;
        const int* first = a.w.first + (size_t)b * a.S_pad;
        for (int i = gl; i < Lb; i += G) {
          const int s0 = 2 * i + 1;
          if (!first[s0]) continue;
          float cm = -INFINITY;
          for (int s = s0; s >= 0; s = nxt[s]) cm = fmaxf(cm, al[s] + be[s]);
          float cs = 0.0f;
          if (cm > -INFINITY)
            for (int s = s0; s >= 0; s = nxt[s]) cs += __expf(al[s] + be[s] - cm);
          const int c = lab[s0];
          const float lp = to_f32<T>(lr[c]) - lse;
          const float occ = cm > -INFINITY ? __expf(cm + __logf(cs) + raw - lp) : 0.0f;
          dr[c] = from_f32<T>(g * (__expf(lp) - occ));
        }
      }
    }
    if constexpr (BLOCK) __syncthreads();
  }
}

// ---- greedy collapse --------------------------------------------------------------------------------------------------------------
// frame t survives when t < T_b, a[t] != blank and a[t] != a[t - 1]; survivors keep their order: per wave a ballot and the count of
// set bits below the lane, the waves of a chunk in order, chunks behind a running offset
__global__ __launch_bounds__(256) void ctc_collapse_kernel(const int64_t* am, int64_t lda, const int64_t* input_lengths, int64_t* ids, int64_t ldi,
                                                            int64_t* lengths, int T, int64_t blank, int64_t pad) {
  __shared__ int sh_cnt[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t* a = am + (int64_t)b * lda;
  int64_t* o = ids + (int64_t)b * ldi;
  const int Tb = clamp_len(input_lengths, b, T);
  int run = 0;
  for (int t0 = 0; t0 < Tb; t0 += 256) {                // block-uniform trip count
    const int t = t0 + threadIdx.x;
    int64_t x = blank;
    bool keep = false;
    if (t < Tb) {
      x = a[t];
      keep = x != blank && (t == 0 || x != a[t - 1]);
    }
    const unsigned long long bal = __ballot(keep);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) sh_cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = run, tot = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) off += sh_cnt[w];
      tot += sh_cnt[w];
    }
    if (keep) o[off + below] = x;
    run += tot;
  }
  for (int t = run + threadIdx.x; t < T; t += 256) o[t] = pad;
  if (threadIdx.x == 0) lengths[b] = run;
}

// ---- prefix beam search -----------------------------------------------------------------------------------------------------------
// launch 1  ctc_beam_prune_kernel  per row (b, t < T_b): row_lse, lp[blank] and the Kc = min(K, C - 1) non-blank classes with the largest
//                                  RAW logit (equal logits by ascending id: fk_beam_topk's rule), as (lp, id) in that order
// launch 2  ctc_beam_kernel        one workgroup per sample, sequential over the frames, the beam in LDS, the prefixes as a trie in the
//                                  workspace; after the last frame the chains are walked backwards into ids
constexpr int BEAM_MAX = 32;                                   // W and K at the top of the envelope
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_ROW = 256;                                  // rows up to this many classes are loaded a frame ahead with the frame's record
static_assert(BEAM_ROW <= BEAM_THREADS, "one class per thread");
constexpr int BEAM_EPT = (BEAM_MAX + BEAM_MAX * BEAM_MAX + BEAM_THREADS - 1) / BEAM_THREADS;   // table entries per thread: 5
constexpr int PRUNE_CAP = 256;                                 // a wave's candidate buffer (keys)
constexpr int PRUNE_U = 4;                                     // vectors a lane loads ahead in the row sweep
static_assert(BEAM_MAX + 64 <= PRUNE_CAP && PRUNE_CAP % 64 == 0, "a compacted buffer takes one more wave of appends");
static_assert(4 * BEAM_MAX <= BEAM_THREADS, "the merge of the four waves' lists: one thread per entry");
static_assert(4 * PRUNE_CAP * sizeof(unsigned long long) <= 16 * 1024, "ctc_beam_prune_kernel: LDS budget");

struct BeamWs {
  float* lse;      // [B T]      row_lse
  float* lpb;      // [B T]      lp[blank]
  float* clp;      // [B T][K]   lp of the candidates, best first; -inf behind the Kc-th
  int* cid;        // [B T][K]   their classes; -1 behind the Kc-th
  int4* nodes;     // [B][T W + 1] the trie: {parent node, label, first child, next sibling}, node 0 the empty prefix
};
static inline size_t beam_ws_carve(BeamWs& w, void* base, int64_t B, int64_t T, int64_t W, int64_t K) {
  char* p = (char*)base;
  size_t o = 0;
  w.lse = (float*)(p + o);  o += a256((size_t)B * T * sizeof(float));
  w.lpb = (float*)(p + o);  o += a256((size_t)B * T * sizeof(float));
  w.clp = (float*)(p + o);  o += a256((size_t)B * T * K * sizeof(float));
  w.cid = (int*)(p + o);    o += a256((size_t)B * T * K * sizeof(int));
  w.nodes = (int4*)(p + o); o += a256((size_t)B * (T * W + 1) * sizeof(int4));
  return o;
}

// a float as an unsigned that orders the same way (-0 ordered as +0: the candidates are ordered by exact float compares)
FK_DEV unsigned f32_ordered(float x) {
  const unsigned u = __float_as_uint(x + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FK_DEV float f32_unordered(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// (value, index) as one key: the larger value first, of equal values the LOWER index; 0 is no entry (no value maps to the high word 0)
FK_DEV unsigned long long beam_key(float x, int idx) { return ((unsigned long long)f32_ordered(x) << 32) | (unsigned)(0x7fffffff - idx); }
FK_DEV int key_index(unsigned long long k) { return 0x7fffffff - (int)(unsigned)(k & 0xffffffffull); }
FK_DEV float key_value(unsigned long long k) { return f32_unordered((unsigned)(k >> 32)); }
// LDS that the lanes of ONE wave hand to each other: the accesses stay in program order for the compiler and the LDS serves a wave's
// instructions in order
FK_DEV void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The wave's buffer buf[0 .. n) of distinct keys -> its K largest, descending, in buf[0 .. min(n, K)); returns the new count.  Rank
// counting: every lane ranks the up to PRUNE_CAP / 64 keys it holds against the whole buffer.
FK_DEV int prune_compact(unsigned long long* buf, int n, int K, int lane) {
  constexpr int Q = PRUNE_CAP / 64;
  unsigned long long mine[Q];
  int rank[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    mine[q] = lane + 64 * q < n ? buf[lane + 64 * q] : 0ull;
    rank[q] = 0;
  }
  for (int i0 = 0; i0 < n; i0 += 8) {                      // eight LDS reads in flight: a read a step would be a chain of LDS latencies
    unsigned long long x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = buf[i0 + u];        // (inside the buffer: PRUNE_CAP is a multiple of 8)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned long long xv = i0 + u < n ? x[u] : 0ull;
#pragma unroll
      for (int q = 0; q < Q; ++q) rank[q] += xv > mine[q] ? 1 : 0;
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (mine[q] != 0ull && rank[q] < K) buf[rank[q]] = mine[q];
  wave_lds_sync();
  return n < K ? n : K;
}

// One wave's view of a row: the candidates that beat the wave's K-th best so far are appended to the wave's LDS buffer in lane order
// (ballot + prefix count); a buffer that could not take another wave of appends is compacted to its K best first, which raises the bar.
struct PruneState {
  unsigned long long* buf;
  unsigned long long bar;     // key of the K-th best so far, 0 while there are fewer
  float bar_x;                // its logit (-inf while there are fewer): the cheap test in front of the keys
  int cnt, K, lane;
};
FK_DEV void prune_push(PruneState& p, float x, int c, bool valid) {   // called by all lanes of the wave together
  if (__ballot(valid && x >= p.bar_x) == 0ull) return;                 // the cheap test: no lane reaches the bar's logit
  unsigned long long key = valid ? beam_key(x, c) : 0ull;
  bool pass = key > p.bar;
  unsigned long long bal = __ballot(pass);
  if (bal == 0ull) return;
  if (p.cnt + 64 > PRUNE_CAP) {
    p.cnt = prune_compact(p.buf, p.cnt, p.K, p.lane);
    if (p.cnt == p.K) { p.bar = p.buf[p.K - 1]; p.bar_x = key_value(p.bar); }
    pass = key > p.bar;
    bal = __ballot(pass);
  }
  if (pass) p.buf[p.cnt + __popcll(bal & ((1ull << p.lane) - 1ull))] = key;
  p.cnt += __popcll(bal);
}

template <typename T, bool BLOCK>
__global__ __launch_bounds__(256) void ctc_beam_prune_kernel(const T* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, BeamWs w,
                                                              int64_t rows, int T_, int C, int blank, int K, int Kc) {
  const RowFrame<T, BLOCK> f{};
  constexpr int N = f.N, G = f.G;
  __shared__ float sh[8];
  __shared__ unsigned long long sh_buf[4][PRUNE_CAP];
  const int gl = f.gl, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = f.first; base < rows; base += f.step) {
    const int64_t row = base + f.sub;
    const bool live = row < rows && (row % T_) < clamp_len(input_lengths, (int)(row / T_), T_);   // wave-uniform; block-uniform under BLOCK
    float m = -INFINITY, s = 0.0f;
    PruneState p{sh_buf[wave], 0ull, -INFINITY, 0, Kc, lane};
    const T* lr = logits;
    if (live) {
      lr = logits + (row / T_) * ldb + (row % T_) * ldt;
      const auto sp = f.split(f.row_head(lr, C), C);
      auto scalars = [&](int c, int end) {              // fewer than N elements: one step of the group
        const bool ok = c < end;
        const float x = ok ? to_f32<T>(lr[c]) : -INFINITY;
        if (ok) lse_push(m, s, x);
        prune_push(p, x, c, ok && c != blank);
      };
      if (sp.head > 0) scalars(gl, sp.head);
      for (int i0 = 0; i0 < sp.nvec; i0 += PRUNE_U * G) {  // wave-uniform trip count: prune_push holds ballots
        float v[PRUNE_U][N];
#pragma unroll
        for (int u = 0; u < PRUNE_U; ++u) {             // PRUNE_U vectors a lane in flight before the first is looked at
          const int i = i0 + u * G + gl;
          if (i < sp.nvec) {
            VecIO<T>::load(lr + sp.head + i * N, v[u]);
          } else {
#pragma unroll
            for (int e = 0; e < N; ++e) v[u][e] = -INFINITY;
          }
        }
#pragma unroll
        for (int u = 0; u < PRUNE_U; ++u) {
          const int i = i0 + u * G + gl, c0 = sp.head + i * N;
          const bool ok = i < sp.nvec;
          const float best = lse_push(m, s, v[u]);     // (a vector behind the row is all -inf: it leaves m and s as they are)
          if (__ballot(ok && best >= p.bar_x) != 0ull) {
#pragma unroll
            for (int e = 0; e < N; ++e) prune_push(p, v[u][e], c0 + e, ok && c0 + e != blank);
          }
        }
      }
      if (sp.tail < C) scalars(sp.tail + gl, C);
      p.cnt = prune_compact(p.buf, p.cnt, Kc, lane);    // the wave's best, descending
      if (lane >= p.cnt && lane < BEAM_MAX) p.buf[lane] = 0ull;
    }
    const float lse = f.finish(m, s, sh);          // its barriers order sh_buf for the merge
    if (live) {
      if (gl == 0) { w.lse[row] = lse; w.lpb[row] = to_f32<T>(lr[blank]) - lse; }
      // the lists of the group's waves merged by rank; a slot behind the Kc-th holds (-inf, -1)
      constexpr int NW = BLOCK ? 4 : 1;
      if (gl < NW * BEAM_MAX) {
        const int lw = BLOCK ? (gl >> 5) : wave, q = gl & (BEAM_MAX - 1);
        const unsigned long long mine = q < Kc ? sh_buf[lw][q] : 0ull;
        int rank = BLOCK ? 0 : q;
        if constexpr (BLOCK) {
          for (int w2 = 0; w2 < 4; ++w2) {
#pragma unroll
            for (int q2 = 0; q2 < BEAM_MAX; ++q2) rank += (q2 < Kc && sh_buf[w2][q2] > mine) ? 1 : 0;   // constant bounds: the reads go out together
          }
        }
        if (mine != 0ull && rank < Kc) {
          w.clp[row * K + rank] = key_value(mine) - lse;
          w.cid[row * K + rank] = key_index(mine);
        }
        if (gl >= Kc && gl < K) { w.clp[row * K + gl] = -INFINITY; w.cid[row * K + gl] = -1; }
      }
    }
    if constexpr (BLOCK) __syncthreads();               // sh_buf is rewritten by the next row
  }
}

struct BeamArgs {
  const void* logits;
  int64_t ldb, ldt;
  const int64_t* input_lengths;
  BeamWs w;
  int64_t* ids;
  int64_t ld_ids_b, ld_ids_h;
  int64_t* lengths;
  float* scores;
  int64_t pad;
  int T, C, blank, W, K, Kc, nbest;
};

FK_DEV float log_add(float a, float b) {
  const float m = fmaxf(a, b);
  return m == -INFINITY ? -INFINITY : m + log1pf(expf(-fabsf(a - b)));
}

// A beam slot is (node, parent node, last label, length, pb, pnb, total); the slots are kept in the order of the selection, total
// descending.  Node ids are canonical: a prefix is looked up among the children of its parent's node before a node is made for it, so a
// prefix that left the beam and is proposed again comes back under the id its descendants still point to, and "candidate (i, c) is beam
// j" is exactly "parent[j] == node[i] and last[j] == c".  The look-up seldom leaves LDS: a slot also carries its node's first child and
// a 64-bit filter of the labels (mod 64) its node ever got a child for, and only a chosen child whose bit is set walks the sibling
// list in the workspace (a node that comes back has lost its filter: all bits set).  Ties of the selection: a resident prefix before
// a new one, then the lower slot / parent slot, then the better candidate (the table index decides).
//
// LM (fk_ctc_beam_search_lm): shallow fusion with a backoff n-gram model.  The acoustic recursion is the one above; a slot also carries
// lmw (the weighted LM term of its prefix), lm (the unweighted sum) and the LM state of its prefix, and the selection runs on
// total + lmw.  A fresh candidate's term comes from one look-up (state of slot i, candidate k), made for the whole table right behind the
// frame's first barrier, so that the waves without resident prefixes look up while the first wave runs the resident step; the values of
// the chosen entries are picked up again from LDS when the next beam is built.  A resident prefix keeps its own values, and a prefix that
// returns is the same sum from the same parent value.  The plain instantiation holds none of this: same LDS, same code as without it.
struct BeamLmArgs : BeamArgs {
  const int4* table;      // [cap] {state, token, bits of ln p, next state}, state -1: empty
  const float* bow;       // [S]
  const int* backoff;     // [S]
  const float* uni_lp;    // [C + 1]
  const int* uni_next;    // [C + 1]
  float* lm_out;          // [B, nbest]
  float* total_out;       // [B, nbest]
  float lm_weight, length_bonus;
  int S, cap_mask, max_probe, order, start_state, use_eos;
};

// the home slot of (state, token) is ngram_hash & (cap - 1): fk_ngram_hash of include/franken_hip.h
__host__ __device__ inline unsigned ngram_hash(unsigned state, unsigned token) {
  unsigned h = state * 0x9E3779B1u ^ token * 0x85EBCA6Bu;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}
FK_DEV int clamp_state(int s, int S) { return s < 0 ? 0 : (s >= S ? S - 1 : s); }
// w lp + bonus, rounded after the product and after the sum: the term has the same bits wherever it is formed
FK_DEV float lm_term(float w, float lp, float bonus) {
#pragma clang fp contract(off)
  const float p = w * lp;
  return p + bonus;
}

// N look-ups side by side.  A look-up is a chain of dependent loads, so everything whose address is known goes out at once: the unigram
// of the token at the start, and per step of a look-up LM_AHEAD consecutive entries of the probe sequence (linear probing: their
// addresses follow from the first) with the state's backoff weight and backoff state; a round is then one load latency unless a probe
// sequence is longer than LM_AHEAD.  The entries are looked at in probe order, none behind max_probe.  Every loop is bounded by
// order * max_probe steps, every state read from a table is clamped into [0, S), a token into [0, C] and a table index by the mask: a
// malformed table gives wrong scores, never an access outside the tables.
//   at most `order` rounds: state 0 -> the dense table; else probe at most max_probe entries from the hash slot: a hit gives
//   (acc + ln p, next), an empty entry or the last probe ends the round with acc += bow[s], s = backoff[s]; behind the last round: unigram
constexpr int LM_AHEAD = 4;                            // (768 x 41, W 32, order 3: 25.6 ms with 1, 21.6 ms with 2, 19.6 ms with 4)
template <int N>
FK_DEV void lm_lookup(const BeamLmArgs& a, const int (&state)[N], const int (&token)[N], const bool (&want)[N], float (&lp)[N], int (&next)[N]) {
  int s[N], tok[N], p[N], rd[N], unx[N];
  float acc[N], ulp[N];
  bool open[N];
#pragma unroll
  for (int r = 0; r < N; ++r) {
    s[r] = clamp_state(state[r], a.S);
    tok[r] = token[r] < 0 ? 0 : (token[r] > a.C ? a.C : token[r]);
    p[r] = 0; rd[r] = 0; acc[r] = 0.0f;
    open[r] = want[r];
    lp[r] = 0.0f; next[r] = 0;
    ulp[r] = 0.0f; unx[r] = 0;
    if (want[r]) { ulp[r] = a.uni_lp[tok[r]]; unx[r] = a.uni_next[tok[r]]; }
  }
  const long long steps = (long long)a.order * a.max_probe;
  for (long long it = 0; it < steps; ++it) {
    int4 e[N][LM_AHEAD];
    float bw[N];
    int bk[N];
    bool any = false;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      if (open[r] && s[r] != 0) {
        const unsigned h = ngram_hash((unsigned)s[r], (unsigned)tok[r]) + (unsigned)p[r];
#pragma unroll
        for (int q = 0; q < LM_AHEAD; ++q) e[r][q] = a.table[(h + (unsigned)q) & (unsigned)a.cap_mask];
        bw[r] = a.bow[s[r]];
        bk[r] = a.backoff[s[r]];
        any = true;
      }
    }
    if (!any) break;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      if (open[r] && s[r] != 0) {
        int verdict = 0;                                // 1: hit, 2: the round is over
        int4 hit = make_int4(0, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < LM_AHEAD; ++q) {
          if (verdict == 0) {
            if (p[r] + q >= a.max_probe || e[r][q].x == -1) verdict = 2;
            else if (e[r][q].x == s[r] && e[r][q].y == tok[r]) { verdict = 1; hit = e[r][q]; }
          }
        }
        if (verdict == 1) {
          lp[r] = acc[r] + __int_as_float(hit.z);
          next[r] = clamp_state(hit.w, a.S);
          open[r] = false;
        } else if (verdict == 2 || p[r] + LM_AHEAD >= a.max_probe) {
          acc[r] += bw[r];
          s[r] = (rd[r] + 1 >= a.order) ? 0 : clamp_state(bk[r], a.S);
          rd[r] += 1;
          p[r] = 0;
        } else {
          p[r] += LM_AHEAD;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (open[r]) {
      lp[r] = acc[r] + ulp[r];
      next[r] = clamp_state(unx[r], a.S);
    }
  }
}

// Lexicon (fk_ctc_beam_search_lex): the search over labellings that spell dictionary words.  The acoustic recursion is the one above and
// the LM fields are the LM instantiation's, over WORD ids (the tables of BeamLmArgs hold the word model, its end of sentence is id V); a
// slot also carries the node of the pronunciation trie its unfinished word has reached (0: a word start) and its word count.  A fresh
// candidate c != sep gets a key only if the trie has the child (node of slot i, c): one probe sequence per entry of the table, made where
// the LM instantiation makes its look-ups.  The sep candidate of a slot is admissible at a terminal node; its word is chosen there among
// the node's up to LEX_HOMOPHONES words by one word-LM look-up each, thread 8 i + h homophone h of slot i.  The chosen word of a sep
// node is kept beside the node (nword), so the walk back fills ids and words in one pass.
constexpr int LEX_HOMOPHONES = 8;
constexpr int LEX_AHEAD = 4;                           // entries of a trie probe sequence in flight (768 x 41, W 32, 2000 words: 21.0 ms with 2, 20.8 ms with 4)
static_assert(BEAM_MAX * LEX_HOMOPHONES <= BEAM_THREADS, "one homophone look-up per thread");
struct BeamLexArgs : BeamLmArgs {
  const int4* trie;       // [tcap] {node, class, child, 0}, node -1: empty
  const int2* node_words; // [n_nodes] {first, count} into word_list
  const int* word_list;   // [n_list]
  int* nword;             // [B][T W + 1] beside BeamWs::nodes: the word a sep node closed, -1 for every other node
  int64_t* words;         // [B, nbest, Lw]
  int64_t ld_words_b, ld_words_h;
  int64_t* word_lengths;  // [B, nbest]
  unsigned char* complete;// [B, nbest]
  int sep, V, n_nodes, n_list, tcap_mask, tmax_probe, Lw;
};
FK_DEV int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// N trie look-ups side by side: child (node, class) or -1.  One probe sequence each, LEX_AHEAD entries a step in flight, none behind
// tmax_probe; the loop is bounded by tmax_probe, a table index by the mask and a child read from the table is clamped into [0, n_nodes).
template <int N>
FK_DEV void trie_lookup(const BeamLexArgs& a, const int (&node)[N], const int (&cls)[N], const bool (&want)[N], int (&child)[N]) {
  bool open[N];
#pragma unroll
  for (int r = 0; r < N; ++r) { open[r] = want[r]; child[r] = -1; }
  for (int p = 0; p < a.tmax_probe; p += LEX_AHEAD) {
    int4 e[N][LEX_AHEAD];
    bool any = false;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      if (open[r]) {
        const unsigned h = ngram_hash((unsigned)node[r], (unsigned)cls[r]) + (unsigned)p;
#pragma unroll
        for (int q = 0; q < LEX_AHEAD; ++q) e[r][q] = a.trie[(h + (unsigned)q) & (unsigned)a.tcap_mask];
        any = true;
      }
    }
    if (!any) break;
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
      for (int q = 0; q < LEX_AHEAD; ++q) {
        if (open[r]) {
          if (p + q >= a.tmax_probe || e[r][q].x == -1) open[r] = false;
          else if (e[r][q].x == node[r] && e[r][q].y == cls[r]) { child[r] = clamp_index(e[r][q].z, a.n_nodes); open[r] = false; }
        }
      }
    }
  }
}

// The three sums that are formed for a key and again when the chosen entry becomes a slot: the total of a resident prefix from this
// frame's pb' and pnb'; what slot i (of a beam's last / pb / tot arrays) sends to its extension by class c at log-probability lp (a repeat
// of the last label continues only what ended in a blank); the weighted LM term of a prefix with a token of ln P = lp behind it
FK_DEV float resident_total(float npb, float npnb) { return log_add(npb, npnb); }
FK_DEV float extended_total(int c, const int* last, const float* pb, const float* tot, int i, float lp) {
  return (c == last[i] ? pb[i] : tot[i]) + lp;
}
FK_DEV float extended_lmw(float lmw, float weight, float lp, float bonus) { return lmw + lm_term(weight, lp, bonus); }

template <typename T, bool LM, bool LEX = false>
__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_kernel(std::conditional_t<LEX, BeamLexArgs, std::conditional_t<LM, BeamLmArgs, BeamArgs>> a) {
  static_assert(LM || !LEX, "the lexicon search carries the LM fields");
  constexpr int M = BEAM_MAX;
  constexpr int ML = LM ? M : 1, MC = LM ? M * M : 1;   // (the plain instantiation never names the arrays below: they take no LDS there)
  constexpr int MX = LEX ? M : 1;                       // (nor does any but the lexicon instantiation name these)
  __shared__ int s_lex[2][MX], s_wc[2][MX];             // per slot: the trie node of its unfinished word, its word count
  __shared__ float s_seplp[MX];                         // this frame's sep extension of slot i: ln P(w* | word state),
  __shared__ int s_sepnx[MX], s_sepw[MX];               // the state behind w*, and w* (-1: the node is not terminal, no sep)
  __shared__ int s_fwc[MX], s_fword[MX], s_fdone[MX];   // behind the last frame: word count with the closing word, that word or -1, complete
  __shared__ float s_lmw[2][ML], s_lms[2][ML];          // per slot: the weighted LM term of its prefix, the unweighted sum of ln P
  __shared__ int s_lst[2][ML];                          // its LM state
  __shared__ float s_candlp[MC];                        // this frame's look-ups, entry W + i Kc + k at i Kc + k: ln P(cid[k] | state of slot i)
  __shared__ int s_candnx[MC];                          // and the state behind it
  __shared__ float s_fkey[ML], s_flm[ML];               // the final keys and LM sums (with the end of sentence)
  __shared__ int s_perm[ML];                            // the final order: place -> slot
  static_assert(!LM || (3 * 2 * M + 2 * M * M + 3 * M) * 4 <= 12 * 1024, "ctc_beam_kernel<LM>: LDS budget of the LM state");
  __shared__ int s_node[2][M], s_par[2][M], s_last[2][M], s_len[2][M];
  __shared__ float s_pb[2][M], s_pnb[2][M], s_tot[2][M];
  __shared__ int s_first[2][M];                         // the node's first child, as nodes[node].z
  __shared__ unsigned long long s_kids[2][M];           // bit (label & 63): the node may have a child with that label
  __shared__ float s_npb[M], s_npnb[M];                 // this frame's pb' and pnb' of the resident prefixes
  __shared__ int s_pslot[M], s_ck[M];                   // slot of the parent prefix / rank of the last label among the candidates, -1: none
  __shared__ unsigned s_merged[M];                      // bit k: candidate k of slot i is a resident prefix
  __shared__ float s_clp[2][M], s_fr[2][2];             // the frame's candidates, {lp[blank], row_lse}; double-buffered over t
  __shared__ int s_cid[2][M];
  __shared__ float s_row[2][BEAM_ROW];                  // C <= BEAM_ROW: the frame's logits, for a last label that is no candidate
  __shared__ unsigned long long s_tmax[BEAM_THREADS], s_surv[M * BEAM_EPT + 16], s_selkey[M];   // the selection: see there
  __shared__ int s_selpar[M], s_sellab[M], s_selnode[M], s_selfirst[M];   // the chosen new prefixes: parent slot, label, node, its first child
  static_assert((10 * 2 * M + 2 * M + 3 * M + 4 * M + 4 + 4 * M + 2 * BEAM_ROW) * 4 + (BEAM_THREADS + M * BEAM_EPT + 16 + M) * 8 <= 16 * 1024, "ctc_beam_kernel: LDS budget");
  const int tid = threadIdx.x, b = blockIdx.x, W = a.W, Kc = a.Kc;
  const int Tb = clamp_len(a.input_lengths, b, a.T);
  int4* nodes = a.w.nodes + (size_t)b * ((size_t)a.T * W + 1);
  const T* lg = (const T*)a.logits + (int64_t)b * a.ldb;
  const int64_t row0 = (int64_t)b * a.T;

  // the table of a frame: entries [0, W) are the resident slots, entry W + i Kc + k is candidate k behind slot i
  const int n_ent = W + W * Kc;
  const int n_thr = n_ent < BEAM_THREADS ? n_ent : BEAM_THREADS;   // threads that hold a key
  int ei[BEAM_EPT], ek[BEAM_EPT];
#pragma unroll
  for (int r = 0; r < BEAM_EPT; ++r) {
    const int e = tid + BEAM_THREADS * r;
    const bool fresh = e >= W && e < n_ent;
    ei[r] = fresh ? (e - W) / Kc : -1;
    ek[r] = fresh ? (e - W) % Kc : 0;
  }
  if (tid < M) {
    s_node[0][tid] = 0; s_par[0][tid] = -1; s_last[0][tid] = -1; s_len[0][tid] = 0;
    s_pb[0][tid] = 0.0f; s_pnb[0][tid] = -INFINITY; s_tot[0][tid] = 0.0f; s_first[0][tid] = -1; s_kids[0][tid] = 0ull;
    s_cid[0][tid] = s_cid[1][tid] = -1;                 // the frames write [0, Kc)
    if constexpr (LM) { s_lmw[0][tid] = 0.0f; s_lms[0][tid] = 0.0f; s_lst[0][tid] = clamp_state(a.start_state, a.S); }
    if constexpr (LEX) { s_lex[0][tid] = 0; s_wc[0][tid] = 0; }
  }
  if (tid == 0) nodes[0] = make_int4(-1, -1, -1, -1);
  [[maybe_unused]] int* nword = nullptr;
  [[maybe_unused]] std::conditional_t<LEX, BeamLmArgs, int> wlm{};                   // lexicon: the word model's view of the arguments (tokens are clamped into [0, V])
  if constexpr (LEX) {
    nword = a.nword + (size_t)b * ((size_t)a.T * W + 1);
    if (tid == 0) nword[0] = -1;
    wlm = a;
    wlm.C = a.V;
  }
  int cur = 0, nb = 1;

  // the frame's record is loaded one frame ahead: threads [0, Kc) a candidate each, thread M lp[blank], thread M + 1 row_lse
  float pf_f = 0.0f, pf_x = 0.0f;
  int pf_i = 0;
  const bool small_row = a.C <= BEAM_ROW;
  auto fetch = [&](int t) {
    const int64_t row = row0 + t;
    if (small_row && tid < a.C) pf_x = to_f32<T>(lg[(int64_t)t * a.ldt + tid]);
    if (tid < Kc) { pf_f = a.w.clp[row * a.K + tid]; pf_i = a.w.cid[row * a.K + tid]; }
    else if (tid == M) pf_f = a.w.lpb[row];
    else if (tid == M + 1) pf_f = a.w.lse[row];
  };
  // The W largest of the table's keys -> their number; leaves the key of rank r in s_selkey[r] and in thread r's mysel.  Only the W
  // threads with the largest own maximum can hold one of them: every thread ranks its maximum among the BEAM_THREADS maxima, those W
  // threads lay all their keys out, and the at most W BEAM_EPT keys laid out are ranked among themselves.  Three barriers whatever W is; keys are distinct, so ranks are.
  auto select = [&](const unsigned long long (&key)[BEAM_EPT], unsigned long long& mysel) {
    unsigned long long mx = key[0];
#pragma unroll
    for (int q = 1; q < BEAM_EPT; ++q) mx = key[q] > mx ? key[q] : mx;
    s_tmax[tid] = mx;
    if (tid < M * BEAM_EPT + 16) s_surv[tid] = 0ull;
    if (tid < M) s_selkey[tid] = 0ull;
    __syncthreads();
    if (mx != 0ull) {
      int rank = 0;
      for (int i0 = 0; i0 < n_thr; i0 += 16) {            // (threads behind the table hold 0; sixteen LDS reads go out together)
#pragma unroll
        for (int u = 0; u < 16; ++u) rank += s_tmax[i0 + u] > mx ? 1 : 0;
      }
      if (rank < W) {
#pragma unroll
        for (int q = 0; q < BEAM_EPT; ++q) s_surv[rank * BEAM_EPT + q] = key[q];
      }
    }
    __syncthreads();
    if (tid < W * BEAM_EPT) {
      const unsigned long long mine = s_surv[tid];
      if (mine != 0ull) {
        int rank = 0;
        for (int i0 = 0; i0 < W * BEAM_EPT; i0 += 16) {   // (what is not laid out is 0)
#pragma unroll
          for (int u = 0; u < 16; ++u) rank += s_surv[i0 + u] > mine ? 1 : 0;
        }
        if (rank < W) s_selkey[rank] = mine;
      }
    }
    __syncthreads();
    mysel = tid < M ? s_selkey[tid] : 0ull;
    return __popcll(__ballot((tid & 63) < W && s_selkey[tid & 63] != 0ull));   // the same in every wave
  };
  // Nodes of the new prefixes (thread r < nsel: chosen entry sel_e): thread i looks its slot's chosen children up among the children of
  // node[i] and makes what is missing; leaves s_selpar / lab / node / first and the slots' first child and filter up to date.
  auto make_nodes = [&](int t, int f, int cur, int nb, int nsel, int sel_e) {
    if (tid < nsel) {
      const bool fresh = sel_e >= W;
      s_selpar[tid] = fresh ? (sel_e - W) / Kc : -1;
      s_sellab[tid] = fresh ? s_cid[f][(sel_e - W) % Kc] : -1;
      s_selnode[tid] = -1;
      s_selfirst[tid] = -1;
    }
    __syncthreads();
    if (tid < nb) {
      unsigned long long want = 0ull;                   // the labels of this slot's chosen children
      unsigned mine = 0u;                               // bit r: chosen entry r is a child of this slot
      int lab[M];
#pragma unroll
      for (int r = 0; r < M; ++r) {                     // constant bounds: the LDS reads go out together
        lab[r] = s_sellab[r];
        if (r < nsel && s_selpar[r] == tid) { mine |= 1u << r; want |= 1ull << (lab[r] & 63); }
      }
      if (mine != 0u) {                                 // (a thread without chosen children does not touch the trie)
        const int n = s_node[cur][tid], first = s_first[cur][tid];
        unsigned found = 0u;
        if (want & s_kids[cur][tid]) {                  // one of them may have a node already
          for (int ch = first; ch >= 0;) {
            const int4 nd = nodes[ch];
#pragma unroll
            for (int r = 0; r < M; ++r)
              if (((mine >> r) & 1u) && lab[r] == nd.y) { s_selnode[r] = ch; s_selfirst[r] = nd.z; found |= 1u << r; }
            ch = nd.w;
          }
        }
        int head = first;
#pragma unroll
        for (int r = 0; r < M; ++r)
          if (((mine & ~found) >> r) & 1u) {
            const int id = 1 + t * W + r;               // <= T W: inside the sample's table
            nodes[id] = make_int4(n, lab[r], -1, head);
            head = id;
            s_selnode[r] = -2 - id;                     // made here (the build step below tells it from a node that came back)
          }
        if (head != first) { nodes[n].z = head; s_first[cur][tid] = head; }
        s_kids[cur][tid] |= want;
      }
    }
    __syncthreads();
  };
  // Lexicon: the word a sep behind slot i closes, w* = argmax over the words of the slot's node of ln P(w | word state), exact ties to
  // the first of the node's list.  Thread 8 i + h looks homophone h up (`gate`: the same in all threads); the 8 lanes of a slot sit in
  // one wave.  Leaves s_seplp / s_sepnx / s_sepw[i] (-1: no word ends at the node).  A list index is clamped into [0, n_list), a word
  // into [0, V), a count into [0, 8]; the root never ends a word.
  auto choose_words = [&](int cur, int nb, bool gate) {
    if constexpr (LEX) {
      const int i = tid / LEX_HOMOPHONES, h = tid % LEX_HOMOPHONES;
      const bool live = gate && i < nb;
      const int n = live ? clamp_index(s_lex[cur][i], a.n_nodes) : 0;
      int2 nw = make_int2(0, 0);
      if (n > 0) nw = a.node_words[n];
      const int cnt = nw.y < 0 ? 0 : (nw.y > LEX_HOMOPHONES ? LEX_HOMOPHONES : nw.y);
      const bool want[1] = {h < cnt};
      const int wd = want[0] ? clamp_index(a.word_list[clamp_index(nw.x + h, a.n_list)], a.V) : 0;
      const int st[1] = {live ? s_lst[cur][i] : 0}, tk[1] = {wd};
      float lp[1];
      int nx_[1];
      lm_lookup<1>(wlm, st, tk, want, lp, nx_);
      float best = want[0] ? lp[0] : -INFINITY;
      int bh = h;
#pragma unroll
      for (int d = 1; d < LEX_HOMOPHONES; d <<= 1) {    // (every lane of the wave is here: no lane left above)
        const float ol = __shfl_xor(best, d);
        const int oh = __shfl_xor(bh, d);
        if (ol > best || (ol == best && oh < bh)) { best = ol; bh = oh; }
      }
      const int src = (tid & 63 & ~(LEX_HOMOPHONES - 1)) + bh;
      const int bnx = __shfl(nx_[0], src), bw = __shfl(wd, src);
      if (h == 0) { s_seplp[i] = best; s_sepnx[i] = bnx; s_sepw[i] = cnt > 0 ? bw : -1; }
    }
  };
  // Lexicon, behind the last frame: a hypothesis at the root is complete; one at a terminal node is closed as if by a sep without an
  // acoustic term (its word, LM term, bonus and state) and is complete; any other is incomplete and keeps its key.  Complete ones add
  // the end of sentence under use_eos.  The order: complete first, then the final key, equal keys in the order of the last selection.
  auto lex_rerank = [&](int cur, int nb) {
    if constexpr (LEX) {
      choose_words(cur, nb, true);
      __syncthreads();
      if (tid < M) {
        float key = -INFINITY, lm = -INFINITY;
        int done = 0, wc = 0, word = -1;
        if (tid < nb) {
          float lmw = s_lmw[cur][tid];
          int st1 = s_lst[cur][tid];
          lm = s_lms[cur][tid];
          wc = s_wc[cur][tid];
          done = s_lex[cur][tid] == 0;
          if (!done && s_sepw[tid] >= 0) {
            lmw = extended_lmw(lmw, a.lm_weight, s_seplp[tid], a.length_bonus);
            lm += s_seplp[tid];
            st1 = s_sepnx[tid];
            word = s_sepw[tid];
            wc += 1;
            done = 1;
          }
          key = s_tot[cur][tid] + lmw;
          if (a.use_eos && done) {
            const int st[1] = {st1}, tk[1] = {a.V};
            const bool want[1] = {true};
            float lp[1];
            int nx_[1];
            lm_lookup<1>(wlm, st, tk, want, lp, nx_);
            key += lm_term(a.lm_weight, lp[0], 0.0f);
            lm += lp[0];
          }
        }
        s_fkey[tid] = key;
        s_flm[tid] = lm;
        s_fdone[tid] = done;
        s_fwc[tid] = wc;
        s_fword[tid] = word;
        s_perm[tid] = tid;
      }
      __syncthreads();
      if (tid < nb) {
        const float mine = s_fkey[tid];
        const int md = s_fdone[tid];
        int rank = 0;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const bool ahead = s_fdone[j] != md ? s_fdone[j] > md : (s_fkey[j] > mine || (s_fkey[j] == mine && j < tid));
          rank += (j < nb && ahead) ? 1 : 0;
        }
        s_perm[rank] = tid;
      }
      __syncthreads();
    }
  };
  // LM, behind the last frame: the final key total + lmw, with use_eos + lm_weight ln P(</s> | state); the beam is put in the order of these keys once more,
  // equal keys in the order of the last selection (s_perm: place -> slot, the identity wherever no rank lands)
  auto lm_rerank = [&](int cur, int nb) {
    if constexpr (LM && !LEX) {
      if (tid < M) {
        float key = -INFINITY, lm = -INFINITY;
        if (tid < nb) {
          key = s_tot[cur][tid] + s_lmw[cur][tid];
          lm = s_lms[cur][tid];
          if (a.use_eos) {
            const int st[1] = {s_lst[cur][tid]}, tk[1] = {a.C};
            const bool want[1] = {true};
            float lp[1];
            int nx_[1];
            lm_lookup<1>(a, st, tk, want, lp, nx_);
            key += lm_term(a.lm_weight, lp[0], 0.0f);
            lm += lp[0];
          }
        }
        s_fkey[tid] = key;
        s_flm[tid] = lm;
        s_perm[tid] = tid;
      }
      __syncthreads();
      if (tid < nb) {
        const float mine = s_fkey[tid];
        int rank = 0;
#pragma unroll
        for (int j = 0; j < M; ++j) rank += (j < nb && (s_fkey[j] > mine || (s_fkey[j] == mine && j < tid))) ? 1 : 0;   // < nb
        s_perm[rank] = tid;
      }
      __syncthreads();
    }
  };
  // The result: slot h is hypothesis h (LM: slot s_perm[h]); its chain is walked backwards into ids.
  auto write_out = [&](int cur, int nb) {
    auto slot_of = [&](int h) {
      if constexpr (LM) return s_perm[h];
      else return h;
    };
    for (int64_t i = tid; i < (int64_t)a.nbest * a.T; i += BEAM_THREADS) {
      const int h = (int)(i / a.T), pos = (int)(i % a.T);
      if (pos >= (h < nb ? s_len[cur][slot_of(h)] : 0)) a.ids[(int64_t)b * a.ld_ids_b + (int64_t)h * a.ld_ids_h + pos] = a.pad;
    }
    if (tid < a.nbest) {
      const bool have = tid < nb;
      const int sl = slot_of(tid);
      const int len = have ? s_len[cur][sl] : 0;
      a.lengths[(int64_t)b * a.nbest + tid] = len;
      a.scores[(int64_t)b * a.nbest + tid] = have ? s_tot[cur][sl] : -INFINITY;
      if constexpr (LM) {
        a.lm_out[(int64_t)b * a.nbest + tid] = have ? s_flm[sl] : -INFINITY;
        a.total_out[(int64_t)b * a.nbest + tid] = have ? s_fkey[sl] : -INFINITY;
      }
      int64_t* o = a.ids + (int64_t)b * a.ld_ids_b + (int64_t)tid * a.ld_ids_h;
      int n = have ? s_node[cur][sl] : 0;
      if constexpr (LEX) {                              // the same walk fills the words: a sep node holds the word it closed
        int64_t* ow = a.words + (int64_t)b * a.ld_words_b + (int64_t)tid * a.ld_words_h;
        int wn = have ? s_fwc[sl] : 0;
        wn = wn > a.Lw ? a.Lw : wn;
        a.word_lengths[(int64_t)b * a.nbest + tid] = wn;
        a.complete[(int64_t)b * a.nbest + tid] = have ? (unsigned char)s_fdone[sl] : 0;
        for (int j = wn; j < a.Lw; ++j) ow[j] = a.pad;
        int wp = wn;
        if (have && s_fword[sl] >= 0 && wp > 0) ow[--wp] = s_fword[sl];
        for (int s = len - 1; s >= 0 && n > 0; --s) {
          const int4 nd = nodes[n];
          const int wd = nword[n];
          o[s] = nd.y;
          if (wd >= 0 && wp > 0) ow[--wp] = wd;
          n = nd.x;
        }
        for (int j = 0; j < wp; ++j) ow[j] = a.pad;     // (only a malformed table leaves a gap)
      } else {
        for (int s = len - 1; s >= 0 && n > 0; --s) {
          const int4 nd = nodes[n];
          o[s] = nd.y;
          n = nd.x;
        }
      }
    }
  };
  // the frames, as tests/ctc_beam_ref.py walks them: record, (LM look-ups,) resident step, keys, select, nodes, next beam
  if (Tb > 0) fetch(0);

  for (int t = 0; t < Tb; ++t) {
    const int f = t & 1;
    if (tid < Kc) { s_clp[f][tid] = pf_f; s_cid[f][tid] = pf_i; }
    else if (tid == M || tid == M + 1) s_fr[f][tid - M] = pf_f;
    if (small_row && tid < a.C) s_row[f][tid] = pf_x;
    __syncthreads();                                    // the record; the beam the last frame left
    if (t + 1 < Tb) fetch(t + 1);

    // LM: ln P(candidate k | state of slot i) for every fresh entry of the table, kept for the keys and laid out for the build step
    float cand_lp[BEAM_EPT];
    [[maybe_unused]] int cand_child[BEAM_EPT];          // lexicon: the trie node behind a fresh entry that is no sep, -1: the lexicon has none
    if constexpr (LEX) {
      int nd[BEAM_EPT], cl[BEAM_EPT];
      bool want[BEAM_EPT];
#pragma unroll
      for (int r = 0; r < BEAM_EPT; ++r) {
        const bool fresh = ei[r] >= 0 && ei[r] < nb;
        cl[r] = fresh ? s_cid[f][ek[r]] : 0;
        nd[r] = fresh ? s_lex[cur][ei[r]] : 0;
        want[r] = fresh && cl[r] != a.sep;
        cand_lp[r] = 0.0f;
      }
      trie_lookup<BEAM_EPT>(a, nd, cl, want, cand_child);
#pragma unroll
      for (int r = 0; r < BEAM_EPT; ++r)
        if (want[r]) s_candnx[ei[r] * Kc + ek[r]] = cand_child[r];
      bool sep_cand = false;
#pragma unroll
      for (int k = 0; k < M; ++k) sep_cand |= s_cid[f][k] == a.sep;                         // (entries behind Kc hold -1)
      choose_words(cur, nb, sep_cand);
    } else if constexpr (LM) {
      int st[BEAM_EPT], tk[BEAM_EPT], nx_[BEAM_EPT];
      bool want[BEAM_EPT];
#pragma unroll
      for (int r = 0; r < BEAM_EPT; ++r) {
        want[r] = ei[r] >= 0 && ei[r] < nb;
        st[r] = want[r] ? s_lst[cur][ei[r]] : 0;
        tk[r] = want[r] ? s_cid[f][ek[r]] : 0;
      }
      lm_lookup<BEAM_EPT>(a, st, tk, want, cand_lp, nx_);
#pragma unroll
      for (int r = 0; r < BEAM_EPT; ++r)
        if (want[r]) { s_candlp[ei[r] * Kc + ek[r]] = cand_lp[r]; s_candnx[ei[r] * Kc + ek[r]] = nx_[r]; }
    }

    // resident prefixes: blank, the repeat of the last label, and what the parent prefix sends through that label
    if (tid < nb) {
      const int j = tid, e = s_last[cur][j];
      int ck = -1, ps = -1;
      float lp_e = -INFINITY, npnb = -INFINITY;
      if (e >= 0) {
#pragma unroll
        for (int k = 0; k < M; ++k) ck = s_cid[f][k] == e ? k : ck;                       // (entries behind Kc hold -1)
        lp_e = ck >= 0 ? s_clp[f][ck] : (small_row ? s_row[f][e] : to_f32<T>(lg[(int64_t)t * a.ldt + e])) - s_fr[f][1];
        npnb = s_pnb[cur][j] + lp_e;
        const int par = s_par[cur][j];
#pragma unroll
        for (int i = 0; i < M; ++i) ps = (i < nb && s_node[cur][i] == par) ? i : ps;
        if (ps >= 0) npnb = log_add(npnb, extended_total(e, s_last[cur], s_pb[cur], s_tot[cur], ps, lp_e));
      }
      s_npb[j] = s_tot[cur][j] + s_fr[f][0];
      s_npnb[j] = npnb;
      s_pslot[j] = ps;
      s_ck[j] = ck;
    }
    __syncthreads();
    if (tid < nb) {
      unsigned mk = 0u;
#pragma unroll
      for (int j = 0; j < M; ++j) mk |= (j < nb && s_pslot[j] == tid && s_ck[j] >= 0) ? (1u << s_ck[j]) : 0u;
      s_merged[tid] = mk;
    }
    __syncthreads();

    // the table's keys, in registers
    unsigned long long key[BEAM_EPT];
#pragma unroll
    for (int r = 0; r < BEAM_EPT; ++r) {
      const int e = tid + BEAM_THREADS * r;
      float v = -INFINITY;
      if (e < nb) {
        v = resident_total(s_npb[e], s_npnb[e]);
        if constexpr (LM) v = v > -INFINITY ? v + s_lmw[cur][e] : v;
      } else if (ei[r] >= 0 && ei[r] < nb) {
        const int i = ei[r], k = ek[r];
        if (!((s_merged[i] >> k) & 1u)) v = extended_total(s_cid[f][k], s_last[cur], s_pb[cur], s_tot[cur], i, s_clp[f][k]);
        if constexpr (LEX) {                            // a candidate the lexicon rejects has no key; only a sep moves the LM term
          const bool is_sep = s_cid[f][k] == a.sep;
          const bool ok = is_sep ? s_sepw[i] >= 0 : cand_child[r] >= 0;
          const float lmw = is_sep ? extended_lmw(s_lmw[cur][i], a.lm_weight, s_seplp[i], a.length_bonus) : s_lmw[cur][i];
          v = (ok && v > -INFINITY) ? v + lmw : -INFINITY;
        } else if constexpr (LM) v = v > -INFINITY ? v + extended_lmw(s_lmw[cur][i], a.lm_weight, cand_lp[r], a.length_bonus) : v;
      }
      key[r] = v > -INFINITY ? beam_key(v, e) : 0ull;   // (a NaN total is no entry either)
    }

    unsigned long long mysel;
    const int nsel = select(key, mysel);
    const int sel_e = tid < nsel ? key_index(mysel) : 0;
    make_nodes(t, f, cur, nb, nsel, sel_e);

    // the next beam, in the order of the selection
    const int nx = cur ^ 1;
    if (tid < nsel) {
      float tot = key_value(mysel);
      if constexpr (LM) {                               // the key is total + lmw there: the total is formed again
        if (sel_e < W) {
          tot = resident_total(s_npb[sel_e], s_npnb[sel_e]);
          s_lmw[nx][tid] = s_lmw[cur][sel_e]; s_lms[nx][tid] = s_lms[cur][sel_e]; s_lst[nx][tid] = s_lst[cur][sel_e];
          if constexpr (LEX) { s_lex[nx][tid] = s_lex[cur][sel_e]; s_wc[nx][tid] = s_wc[cur][sel_e]; }
        } else {
          const int i = s_selpar[tid], k = (sel_e - W) % Kc;
          if constexpr (LEX) {
            tot = extended_total(s_cid[f][k], s_last[cur], s_pb[cur], s_tot[cur], i, s_clp[f][k]);
            const bool is_sep = s_cid[f][k] == a.sep;
            s_lmw[nx][tid] = is_sep ? extended_lmw(s_lmw[cur][i], a.lm_weight, s_seplp[i], a.length_bonus) : s_lmw[cur][i];
            s_lms[nx][tid] = is_sep ? s_lms[cur][i] + s_seplp[i] : s_lms[cur][i];
            s_lst[nx][tid] = is_sep ? s_sepnx[i] : s_lst[cur][i];
            s_lex[nx][tid] = is_sep ? 0 : s_candnx[sel_e - W];
            s_wc[nx][tid] = s_wc[cur][i] + (is_sep ? 1 : 0);
            const int nd = s_selnode[tid], id = nd < -1 ? -2 - nd : nd;   // <= T W: inside the sample's table
            if (id >= 0) nword[id] = is_sep ? s_sepw[i] : -1;             // (a node that came back holds the same word already)
          } else {
            const float lp = s_candlp[sel_e - W];
            tot = extended_total(s_cid[f][k], s_last[cur], s_pb[cur], s_tot[cur], i, s_clp[f][k]);
            s_lmw[nx][tid] = extended_lmw(s_lmw[cur][i], a.lm_weight, lp, a.length_bonus);
            s_lms[nx][tid] = s_lms[cur][i] + lp;
            s_lst[nx][tid] = s_candnx[sel_e - W];
          }
        }
      }
      if (sel_e < W) {
        s_node[nx][tid] = s_node[cur][sel_e]; s_par[nx][tid] = s_par[cur][sel_e]; s_last[nx][tid] = s_last[cur][sel_e];
        s_len[nx][tid] = s_len[cur][sel_e]; s_pb[nx][tid] = s_npb[sel_e]; s_pnb[nx][tid] = s_npnb[sel_e];
        s_first[nx][tid] = s_first[cur][sel_e]; s_kids[nx][tid] = s_kids[cur][sel_e];
      } else {
        const int i = s_selpar[tid], nd = s_selnode[tid];
        const bool made = nd < -1;
        s_node[nx][tid] = made ? -2 - nd : nd; s_par[nx][tid] = s_node[cur][i]; s_last[nx][tid] = s_sellab[tid];
        s_len[nx][tid] = s_len[cur][i] + 1; s_pb[nx][tid] = -INFINITY; s_pnb[nx][tid] = tot;
        s_first[nx][tid] = made ? -1 : s_selfirst[tid]; s_kids[nx][tid] = made ? 0ull : ~0ull;
      }
      s_tot[nx][tid] = tot;
    }
    cur = nx;
    nb = nsel;
  }
  __syncthreads();
  lm_rerank(cur, nb);
  lex_rerank(cur, nb);
  write_out(cur, nb);
}

// The route of a row-parallel kernel (a template over <T, BLOCK>; TT names the dtype in its arguments): a row of more than 1024 classes
// takes a workgroup, a shorter one a wave, four rows a workgroup; at most 8192 workgroups walk the rows.
#define CTC_LAUNCH_ROWS(kernel, dtype, rows, C, stream, ...)                                                                           \
  do {                                                                                                                                  \
    const bool block__ = (C) > 1024;                                                                                                    \
    const int64_t wgs__ = block__ ? (rows) : fk_cdiv((rows), 4);                                                                        \
    const dim3 grid__((unsigned)(wgs__ < 8192 ? wgs__ : 8192));                                                                         \
    if (block__) FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((kernel<TT, true>), grid__, dim3(256), 0, stream, __VA_ARGS__));             \
    else FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((kernel<TT, false>), grid__, dim3(256), 0, stream, __VA_ARGS__));                    \
  } while (0)

// The checks every entry point over logits [B, T, C] makes first, under the caller's name (`pointers`: its own are all there).  The
// stride checks stay with the callers: each message names the caller's other strides, behind the caller's envelope checks.
static int check_common(const char* fn, int dtype, bool pointers, int64_t B, int64_t T, int64_t C, int64_t blank) {
  FK_CHECK_ARG(dtype == FK_F32 || dtype == FK_BF16, "%s: bad dtype %d", fn, dtype);
  FK_CHECK_ARG(pointers, "%s: null pointer", fn);
  FK_CHECK_ARG(B > 0 && T > 0 && B * T < (1LL << 31), "%s: B = %lld, T = %lld", fn, (long long)B, (long long)T);
  FK_CHECK_ARG(C >= 2 && C < (1LL << 31), "%s: C = %lld, must be >= 2 (a class beside the blank)", fn, (long long)C);
  FK_CHECK_ARG(blank >= 0 && blank < C, "%s: blank = %lld outside [0, C = %lld)", fn, (long long)blank, (long long)C);
  return FK_OK;
}

// ---- prefix scores for joint CTC / attention decoding (the rule: include/franken_hip.h; float64 restatement tests/ctc_prefix_ref.py) ----
// One wave per row of the GPT beam search.  A hypothesis' state r_n / r_b [T] sits in LDS; the kernels recompute instead of storing every
// candidate's state: the score of a candidate needs no recursion (psi' = logsumexp_t(phi[t] + y[t][c]), phi from the hypothesis alone), so
// the k candidates sit on the lanes and sweep the frames with CTC_PF gathers in flight, and only the one extension the select chose
// (pfx_extend) walks the frames in order, on one lane, from operands the wave has staged in LDS.
constexpr int PFX_MAX_T = 1024, PFX_MAX_K = 64, PFX_MAX_W = 16, PFX_MAX_PROMPT = 64;
constexpr int PFX_NONE = -1, PFX_BAD = -2;             // `last` of the empty hypothesis / of one that took a label outside the classes

struct PfxLds { float n[PFX_MAX_T], b[PFX_MAX_T], phi[PFX_MAX_T], y[PFX_MAX_T], yb[PFX_MAX_T], lse[PFX_MAX_T]; };
static_assert(sizeof(PfxLds) <= 32 * 1024, "ctc_prefix kernels: LDS budget");

// log(e^a + e^b); two -inf give -inf, never inf - inf
FK_DEV float lae(float a, float b) {
  const float m = fmaxf(a, b);
  return m == -INFINITY ? -INFINITY : m + __logf(1.0f + __expf(fminf(a, b) - m));
}

// The hypothesis in L.n / L.b (psi, last) takes label c; L.lse and L.yb hold the sentence's row_lse and y[.][blank].  Every lane calls it
// (barriers inside).  A label outside [0, C) or equal to the blank leaves the impossible hypothesis: everything -inf, last = PFX_BAD.
template <typename T>
FK_DEV void pfx_extend(PfxLds& L, const T* lg, int64_t ldt, int Tg, int C, int blank, int64_t c, float& psi, int& last) {
  const int lane = threadIdx.x;
  const bool ok = c >= 0 && c < C && c != blank;
  const bool same = ok && (int)c == last, empty = last == PFX_NONE;
  const T* col = lg + (ok ? c : 0);
  float m = -INFINITY, s = 0.0f;
  for (int t = lane; t < Tg; t += 64) {                 // phi[0] = 0 or -inf stands for n[0] = y[0][c] or -inf
    const float y = ok ? to_f32<T>(col[(int64_t)t * ldt]) - L.lse[t] : -INFINITY;
    const float phi = t == 0 ? (empty ? 0.0f : -INFINITY) : (same ? L.b[t - 1] : lae(L.n[t - 1], L.b[t - 1]));
    L.phi[t] = phi;
    L.y[t] = y;
    lse_push(m, s, phi + y);
  }
  const float M = wave_max(m);
  const float tot = wave_sum(m > -INFINITY ? s * __expf(m - M) : 0.0f);
  psi = M > -INFINITY ? M + logf(tot) : -INFINITY;
  __syncthreads();
  if (lane == 0) {
    float n = -INFINITY, b = -INFINITY;
#pragma unroll 4
    for (int t = 0; t < Tg; ++t) {
      const float nn = lae(n, L.phi[t]) + L.y[t];
      const float bb = t ? lae(n, b) + L.yb[t] : -INFINITY;
      L.n[t] = nn;
      L.b[t] = bb;
      n = nn;
      b = bb;
    }
  }
  __syncthreads();
  last = ok ? (int)c : PFX_BAD;
}

// the state in LDS to row `row` of a state buffer [rows, 2, T]; frames behind the sentence's length get -inf, so every element is written
FK_DEV void pfx_store(const PfxLds& L, float* st, int64_t row, int T, int Tg) {
  float* d = st + row * 2 * T;
  for (int t = threadIdx.x; t < T; t += 64) {
    d[t] = t < Tg ? L.n[t] : -INFINITY;
    d[T + t] = t < Tg ? L.b[t] : -INFINITY;
  }
}

struct PfxInitArgs {
  const void* logits;
  int64_t ldb, ldt;
  const int64_t* input_lengths;
  const float* row_lse;
  const int64_t* prompt;
  int64_t prompt_ld;
  float* st0;
  float* psi;
  int32_t* last;
  int T, C, blank, W, P;
};

template <typename T>
__global__ __launch_bounds__(64) void ctc_prefix_init_kernel(PfxInitArgs a) {
  __shared__ PfxLds L;
  const int lane = threadIdx.x, g = blockIdx.x;
  const int Tg = clamp_len(a.input_lengths, g, a.T);
  const T* lg = (const T*)a.logits + (int64_t)g * a.ldb;
  const float* lse = a.row_lse + (int64_t)g * a.T;
  for (int t = lane; t < Tg; t += 64) {
    L.lse[t] = lse[t];
    L.yb[t] = to_f32<T>(lg[(int64_t)t * a.ldt + a.blank]) - lse[t];
    L.n[t] = -INFINITY;
  }
  __syncthreads();
  if (lane == 0) {                                      // the empty hypothesis: r_b[t] = the blanks of frames 0 .. t, summed in frame order
    float acc = 0.0f;
    for (int t = 0; t < Tg; ++t) { acc += L.yb[t]; L.b[t] = acc; }
  }
  __syncthreads();
  float psi = 0.0f;
  int last = PFX_NONE;
  for (int i = 0; i < a.P; ++i) pfx_extend<T>(L, lg, a.ldt, Tg, a.C, a.blank, a.prompt[(int64_t)g * a.prompt_ld + i], psi, last);
  for (int b = 0; b < a.W; ++b) {
    const int64_t r = (int64_t)g * a.W + b;
    pfx_store(L, a.st0, r, a.T, Tg);
    if (lane == 0) { a.psi[r] = psi; a.last[r] = last; }
  }
}

struct PfxArgs {
  const void* logits;
  int64_t ldb, ldt;
  const int64_t* input_lengths;
  const float* row_lse;
  float* top_lp;
  const int64_t* top_id;
  const int32_t* fin;
  const int64_t* step;
  const int32_t* parent_log;
  const int64_t* tok_log;
  float* st[2];
  float* psi;         // [2][S W], like `last`: the halves swap with the state buffers
  int32_t* last;
  int64_t eos, log_rows;
  float weight;
  int S, T, C, blank, W, k, broadcast;
};

template <typename T>
__global__ __launch_bounds__(64) void ctc_prefix_score_kernel(PfxArgs a) {
  __shared__ PfxLds L;
  const int lane = threadIdx.x, R = a.S * a.W;
  const int g = a.broadcast ? blockIdx.x : blockIdx.x / a.W;
  const int r = a.broadcast ? g * a.W : blockIdx.x;
  const int64_t step = *a.step;
  if (step < 0 || step > a.log_rows) return;
  if (a.fin && a.fin[r]) return;                        // a finished beam: its row of top_lp stays, it carries no state
  const int par = (int)(step & 1);
  const bool advance = !a.broadcast && step > 0;
  const int Tg = clamp_len(a.input_lengths, g, a.T);
  const T* lg = (const T*)a.logits + (int64_t)g * a.ldb;
  const float* lse = a.row_lse + (int64_t)g * a.T;

  // the hypothesis this row continues: its own (first step), or the one the last select made its parent, in the other buffer
  int src_buf = par, src_row = r;
  int64_t tok = 0;
  if (advance) {
    const int64_t o = (step - 1) * R + r;
    const int p = a.parent_log[o];
    src_row = g * a.W + (p < 0 ? 0 : (p >= a.W ? a.W - 1 : p));
    src_buf = par ^ 1;
    tok = a.tok_log[o];
  }
  const float* sn = a.st[src_buf] + (int64_t)src_row * 2 * a.T;
  for (int t = lane; t < Tg; t += 64) {
    L.n[t] = sn[t];
    L.b[t] = sn[a.T + t];
    L.lse[t] = lse[t];
    if (advance) L.yb[t] = to_f32<T>(lg[(int64_t)t * a.ldt + a.blank]) - lse[t];
  }
  float psi = a.psi[src_buf * R + src_row];
  int last = a.last[src_buf * R + src_row];
  __syncthreads();
  if (advance) {
    pfx_extend<T>(L, lg, a.ldt, Tg, a.C, a.blank, tok, psi, last);
    pfx_store(L, a.st[par], r, a.T, Tg);
    if (lane == 0) { a.psi[par * R + r] = psi; a.last[par * R + r] = last; }
  }

  // phi of a label other than `last` (a label equal to it reads r_b[t - 1] directly)
  for (int t = lane; t < Tg; t += 64) L.phi[t] = t ? lae(L.n[t - 1], L.b[t - 1]) : (last == PFX_NONE ? 0.0f : -INFINITY);
  __syncthreads();
  if (lane >= a.k) return;
  const int64_t o = (int64_t)blockIdx.x * a.k + lane;
  const int64_t c = a.top_id[o];
  float delta = FK_CTC_PREFIX_FLOOR;
  if (Tg > 0 && psi > -INFINITY) {
    float psi2 = -INFINITY;
    if (a.eos >= 0 && c == a.eos) {                     // the hypothesis ends here: the probability of the whole labelling
      psi2 = lae(L.n[Tg - 1], L.b[Tg - 1]);
    } else if (c >= 0 && c < a.C && c != a.blank) {
      const bool same = (int)c == last;
      const T* col = lg + c;
      float m = -INFINITY, s = 0.0f;
      for (int t0 = 0; t0 < Tg; t0 += CTC_PF) {
        T raw[CTC_PF];
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) raw[i] = col[(int64_t)(t0 + i < Tg ? t0 + i : Tg - 1) * a.ldt];
        float v[CTC_PF];
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) {
          const int t = t0 + i < Tg ? t0 + i : Tg - 1;
          const float phi = same ? (t ? L.b[t - 1] : -INFINITY) : L.phi[t];
          v[i] = t0 + i < Tg ? phi + (to_f32<T>(raw[i]) - L.lse[t]) : -INFINITY;
        }
        lse_push(m, s, v);
      }
      psi2 = m > -INFINITY ? m + logf(s) : -INFINITY;
    }
    if (psi2 > -INFINITY) delta = psi2 - psi;
  }
  a.top_lp[o] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, a.weight), a.top_lp[o]), __fmul_rn(a.weight, delta));
}

// the checks fk_ctc_prefix_init and fk_ctc_prefix_score share
static int prefix_check(const char* fn, int dtype, bool pointers, int64_t ldb, int64_t ldt, int64_t S, int64_t T, int64_t C, int64_t blank, int64_t W) {
  if (const int rc = check_common(fn, dtype, pointers, S, T, C, blank)) return rc;
  FK_CHECK_ARG(T <= PFX_MAX_T && W >= 1 && W <= PFX_MAX_W && S * W < (1LL << 24), "%s: T = %lld, W = %lld, S = %lld outside the envelope (T <= %d, 1 <= W <= %d)",
               fn, (long long)T, (long long)W, (long long)S, PFX_MAX_T, PFX_MAX_W);
  FK_CHECK_ARG(ldt >= C && ldb >= ldt, "%s: row stride %lld below C = %lld (batch stride %lld)", fn, (long long)ldt, (long long)C, (long long)ldb);
  return FK_OK;
}

// The argument checks, the workspace and launch 1 of fk_ctc_beam_search and fk_ctc_beam_search_lm; fills everything
// of `a` the plain search reads.
static int beam_front(const char* fn, const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t B, int64_t T, int64_t C,
                      int64_t blank, int64_t W, int64_t K, int64_t nbest, int64_t pad, int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h,
                      int64_t* lengths, float* scores, int dtype, void* workspace, size_t workspace_bytes, void* stream, BeamArgs& a) {
  if (const int rc = check_common(fn, dtype, logits && ids && lengths && scores, B, T, C, blank)) return rc;
  FK_CHECK_ARG(W >= 1 && W <= BEAM_MAX && K >= 1 && K <= BEAM_MAX, "%s: W = %lld, K = %lld outside the envelope (1 .. %d each)", fn, (long long)W,
               (long long)K, BEAM_MAX);
  FK_CHECK_ARG(T * W < (1LL << 31) - 1, "%s: T W = %lld nodes per sample", fn, (long long)(T * W));
  FK_CHECK_ARG(nbest >= 1 && nbest <= W, "%s: nbest = %lld outside 1 .. W = %lld", fn, (long long)nbest, (long long)W);
  FK_CHECK_ARG(ldt >= C && ldb >= ldt, "%s: row stride %lld below C = %lld (batch stride %lld)", fn, (long long)ldt, (long long)C, (long long)ldb);
  FK_CHECK_ARG(ld_ids_h >= T && ld_ids_b >= (nbest - 1) * ld_ids_h + T, "%s: ids strides %lld / %lld below [nbest = %lld, T = %lld]", fn,
               (long long)ld_ids_b, (long long)ld_ids_h, (long long)nbest, (long long)T);
  const size_t need = beam_ws_carve(a.w, workspace, B, T, W, K);
  FK_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu bytes, fk_ctc_beam_workspace_bytes gives %zu)", fn, workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = B * T;
  const int Kc = (int)(K < C - 1 ? K : C - 1);
  CTC_LAUNCH_ROWS(ctc_beam_prune_kernel, dtype, rows, C, s, (const TT*)logits, ldb, ldt, input_lengths, a.w, rows, (int)T, (int)C, (int)blank, (int)K, Kc);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fk_set_error(FK_ELAUNCH, "%s(prune): %s", fn, hipGetErrorString(e));
  a.logits = logits; a.ldb = ldb; a.ldt = ldt; a.input_lengths = input_lengths;
  a.ids = ids; a.ld_ids_b = ld_ids_b; a.ld_ids_h = ld_ids_h; a.lengths = lengths; a.scores = scores; a.pad = pad;
  a.T = (int)T; a.C = (int)C; a.blank = (int)blank; a.W = (int)W; a.K = (int)K; a.Kc = Kc; a.nbest = (int)nbest;
  return FK_OK;
}

}  // namespace

extern "C" {

int fk_ctc_route(int64_t Lmax) {
  FK_CHECK_ARG(Lmax >= 0 && 2 * Lmax + 1 <= CTC_MAX_S, "fk_ctc_route: Lmax = %lld outside the envelope (2 * Lmax + 1 <= %d extended states)",
               (long long)Lmax, CTC_MAX_S);
  return 2 * Lmax + 1 <= 64 ? FK_CTC_WAVE : FK_CTC_LDS;
}

size_t fk_ctc_workspace_bytes(int64_t B, int64_t T, int64_t Lmax) {
  if (B <= 0 || T < 0 || Lmax < 0 || 2 * Lmax + 1 > CTC_MAX_S) return 0;
  CtcWs w;
  return ctc_ws_carve(w, nullptr, B, T, ctc_spad(Lmax));
}

int fk_ctc_loss_fwd(const void* logits, int64_t ldb, int64_t ldt, const int64_t* targets, int64_t ldtgt, const int64_t* input_lengths,
                    const int64_t* target_lengths, int64_t pad_value, float* nll, float* loss2, float* row_lse, int64_t B, int64_t T,
                    int64_t C, int64_t Lmax, int64_t blank, int reduction, int zero_infinity, int want_lattice, int dtype, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (const int rc = check_common("fk_ctc_loss_fwd", dtype, logits && nll && loss2 && row_lse && workspace && (targets || Lmax == 0), B, T, C, blank)) return rc;
  FK_CHECK_ARG(Lmax >= 0 && 2 * Lmax + 1 <= CTC_MAX_S, "fk_ctc_loss_fwd: Lmax = %lld outside the envelope (2 * Lmax + 1 <= %d extended states)",
               (long long)Lmax, CTC_MAX_S);
  FK_CHECK_ARG(ldt >= C && ldb >= ldt && ldtgt >= Lmax, "fk_ctc_loss_fwd: row stride %lld below C = %lld (batch stride %lld, target stride %lld)",
               (long long)ldt, (long long)C, (long long)ldb, (long long)ldtgt);
  FK_CHECK_ARG(reduction == FK_CTC_NONE || reduction == FK_CTC_SUM || reduction == FK_CTC_MEAN, "fk_ctc_loss_fwd: reduction %d", reduction);
  CtcFwdArgs a;
  a.S_pad = ctc_spad(Lmax);
  const size_t need = ctc_ws_carve(a.w, workspace, B, want_lattice ? T : 0, a.S_pad);
  FK_CHECK_ARG(workspace_bytes >= need, "fk_ctc_loss_fwd: workspace too small (%zu bytes, fk_ctc_workspace_bytes gives %zu)", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = B * T;
  CTC_LAUNCH_ROWS(ctc_row_lse_kernel, dtype, rows, C, s, (const TT*)logits, ldb, ldt, row_lse, rows, (int)T, (int)C);
  FK_CHECK_LAUNCH("fk_ctc_loss_fwd(row_lse)");
  a.logits = logits; a.ldb = ldb; a.ldt = ldt; a.targets = targets; a.ldtgt = ldtgt;
  a.input_lengths = input_lengths; a.target_lengths = target_lengths; a.pad_value = pad_value;
  a.row_lse = row_lse; a.nll = nll;
  a.T = (int)T; a.C = (int)C; a.Lmax = (int)Lmax; a.blank = (int)blank; a.zero_inf = zero_infinity != 0; a.want_lattice = want_lattice != 0;
  const dim3 grid((unsigned)B, want_lattice ? 2 : 1);
  if (a.S_pad <= 64)
    FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_lattice_kernel<TT, true>), grid, dim3(64), 0, s, a));
  else
    FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_lattice_kernel<TT, false>), grid, dim3(a.S_pad), 0, s, a));
  FK_CHECK_LAUNCH("fk_ctc_loss_fwd(lattice)");
  hipLaunchKernelGGL(ctc_final_kernel, dim3(1), dim3(FK_TPB), 0, s, (const float*)nll, (const int*)a.w.len, loss2, (int)B, reduction);
  FK_CHECK_LAUNCH("fk_ctc_loss_fwd(final)");
  return FK_OK;
}

int fk_ctc_loss_bwd(const void* logits, int64_t ldb, int64_t ldt, const float* row_lse, const float* grad_out, void* dlogits, int64_t lddb,
                    int64_t lddt, int64_t B, int64_t T, int64_t C, int64_t Lmax, int64_t blank, int reduction, int zero_infinity, int dtype,
                    const void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = check_common("fk_ctc_loss_bwd", dtype, logits && row_lse && grad_out && dlogits && workspace, B, T, C, blank)) return rc;
  FK_CHECK_ARG(Lmax >= 0 && 2 * Lmax + 1 <= CTC_MAX_S, "fk_ctc_loss_bwd: Lmax = %lld outside the envelope (2 * Lmax + 1 <= %d extended states)",
               (long long)Lmax, CTC_MAX_S);
  FK_CHECK_ARG(ldt >= C && ldb >= ldt && lddt >= C && lddb >= lddt, "fk_ctc_loss_bwd: row stride %lld / %lld below C = %lld", (long long)ldt,
               (long long)lddt, (long long)C);
  FK_CHECK_ARG(reduction == FK_CTC_NONE || reduction == FK_CTC_SUM || reduction == FK_CTC_MEAN, "fk_ctc_loss_bwd: reduction %d", reduction);
  CtcBwdArgs a;
  a.S_pad = ctc_spad(Lmax);
  const size_t need = ctc_ws_carve(a.w, const_cast<void*>(workspace), B, T, a.S_pad);
  FK_CHECK_ARG(workspace_bytes >= need, "fk_ctc_loss_bwd: workspace too small (%zu bytes, fk_ctc_workspace_bytes gives %zu)", workspace_bytes, need);
  a.logits = logits; a.ldb = ldb; a.ldt = ldt; a.row_lse = row_lse; a.gout = grad_out; a.dl = dlogits; a.lddb = lddb; a.lddt = lddt;
  a.B = (int)B; a.T = (int)T; a.C = (int)C; a.blank = (int)blank; a.reduction = reduction; a.zero_inf = zero_infinity != 0;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = B * T;
  CTC_LAUNCH_ROWS(ctc_bwd_kernel, dtype, rows, C, s, a);
  FK_CHECK_LAUNCH("fk_ctc_loss_bwd");
  return FK_OK;
}

int fk_ctc_collapse(const int64_t* argmax, int64_t lda, const int64_t* input_lengths, int64_t* ids, int64_t ldi, int64_t* lengths, int64_t B,
                    int64_t T, int64_t blank, int64_t pad, void* stream) {
  FK_CHECK_ARG(argmax && ids && lengths, "fk_ctc_collapse: null pointer");
  FK_CHECK_ARG(B > 0 && B < (1LL << 31) && T > 0 && T < (1LL << 31) && lda >= T && ldi >= T, "fk_ctc_collapse: B = %lld, T = %lld, strides %lld / %lld",
               (long long)B, (long long)T, (long long)lda, (long long)ldi);
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, argmax, lda, input_lengths, ids, ldi, lengths, (int)T, blank, pad);
  FK_CHECK_LAUNCH("fk_ctc_collapse");
  return FK_OK;
}

size_t fk_ctc_align_workspace_bytes(int64_t B, int64_t T, int64_t Lmax) {
  if (B <= 0 || T <= 0 || B * T >= (1LL << 31) || Lmax < 0 || 2 * Lmax + 1 > CTC_MAX_S) return 0;
  CtcAlignWs w;
  return align_ws_carve(w, nullptr, B, T, ctc_spad(Lmax));
}

int fk_ctc_align(const void* logits, int64_t ldb, int64_t ldt, const int64_t* targets, int64_t ldtgt, const int64_t* input_lengths,
                 const int64_t* target_lengths, int64_t pad_value, int64_t B, int64_t T, int64_t C, int64_t Lmax, int64_t blank, int64_t pad,
                 float* score, int64_t* path, int64_t ld_path, int64_t* index, int64_t ld_index, int64_t* start, int64_t* end, float* label_lp,
                 int64_t ld_lab, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = check_common("fk_ctc_align", dtype, logits && score && path && (targets || Lmax == 0), B, T, C, blank)) return rc;
  FK_CHECK_ARG(Lmax >= 0 && 2 * Lmax + 1 <= CTC_MAX_S, "fk_ctc_align: Lmax = %lld outside the envelope (2 * Lmax + 1 <= %d extended states)",
               (long long)Lmax, CTC_MAX_S);
  FK_CHECK_ARG(ldt >= C && ldb >= ldt && ldtgt >= Lmax, "fk_ctc_align: row stride %lld below C = %lld (batch stride %lld, target stride %lld)",
               (long long)ldt, (long long)C, (long long)ldb, (long long)ldtgt);
  FK_CHECK_ARG(T < (1LL << 31) - CTC_ALIGN_CHUNK, "fk_ctc_align: T = %lld frames leave no room for the frame index", (long long)T);
  FK_CHECK_ARG(ld_path >= T && (!index || ld_index >= T), "fk_ctc_align: path / index stride %lld / %lld below T = %lld", (long long)ld_path,
               (long long)ld_index, (long long)T);
  FK_CHECK_ARG(!(start || end || label_lp) || ld_lab >= Lmax, "fk_ctc_align: label stride %lld below Lmax = %lld", (long long)ld_lab, (long long)Lmax);
  CtcAlignArgs a;
  a.S_pad = ctc_spad(Lmax);
  const size_t need = align_ws_carve(a.w, workspace, B, T, a.S_pad);
  FK_CHECK_ARG(workspace && workspace_bytes >= need, "fk_ctc_align: workspace too small (%zu bytes, fk_ctc_align_workspace_bytes gives %zu)",
               workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = B * T;
  CTC_LAUNCH_ROWS(ctc_row_lse_kernel, dtype, rows, C, s, (const TT*)logits, ldb, ldt, a.w.row_lse, rows, (int)T, (int)C);
  FK_CHECK_LAUNCH("fk_ctc_align(row_lse)");
  a.logits = logits; a.ldb = ldb; a.ldt = ldt; a.targets = targets; a.ldtgt = ldtgt;
  a.input_lengths = input_lengths; a.target_lengths = target_lengths; a.pad_value = pad_value; a.pad = pad;
  a.score = score; a.path = path; a.ld_path = ld_path; a.index = index; a.ld_index = ld_index;
  a.start = start; a.end = end; a.label_lp = label_lp; a.ld_lab = ld_lab;
  a.T = (int)T; a.C = (int)C; a.Lmax = (int)Lmax; a.blank = (int)blank;
  if (a.S_pad <= 64)
    FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_align_kernel<TT, true>), dim3((unsigned)B), dim3(64), 0, s, a));
  else
    FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_align_kernel<TT, false>), dim3((unsigned)B), dim3(a.S_pad), 0, s, a));
  FK_CHECK_LAUNCH("fk_ctc_align(align)");
  return FK_OK;
}

size_t fk_ctc_beam_workspace_bytes(int64_t B, int64_t T, int64_t W, int64_t K) {
  if (B <= 0 || T <= 0 || W < 1 || W > BEAM_MAX || K < 1 || K > BEAM_MAX) return 0;
  BeamWs w;
  return beam_ws_carve(w, nullptr, B, T, W, K);
}

int fk_ctc_beam_search(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t B, int64_t T, int64_t C, int64_t blank,
                       int64_t W, int64_t K, int64_t nbest, int64_t pad, int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, int64_t* lengths,
                       float* scores, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  BeamArgs a;
  const int rc = beam_front("fk_ctc_beam_search", logits, ldb, ldt, input_lengths, B, T, C, blank, W, K, nbest, pad, ids, ld_ids_b, ld_ids_h, lengths, scores,
                            dtype, workspace, workspace_bytes, stream, a);
  if (rc != FK_OK) return rc;
  FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_beam_kernel<TT, false>), dim3((unsigned)B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, a));
  FK_CHECK_LAUNCH("fk_ctc_beam_search(recursion)");
  return FK_OK;
}

uint32_t fk_ngram_hash(uint32_t state, uint32_t token) { return ngram_hash(state, token); }

int fk_ctc_beam_search_lm(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t B, int64_t T, int64_t C, int64_t blank,
                          int64_t W, int64_t K, int64_t nbest, int64_t pad, const int32_t* lm_table, int64_t lm_cap, int64_t lm_max_probe,
                          const float* lm_bow, const int32_t* lm_backoff, int64_t lm_states, const float* lm_uni_lp, const int32_t* lm_uni_next,
                          int64_t lm_start_state, int64_t lm_order, float lm_weight, float length_bonus, int use_eos, int64_t* ids,
                          int64_t ld_ids_b, int64_t ld_ids_h, int64_t* lengths, float* am, float* lm, float* total, int dtype, void* workspace,
                          size_t workspace_bytes, void* stream) {
  FK_CHECK_ARG(lm_table && lm_bow && lm_backoff && lm_uni_lp && lm_uni_next && lm && total, "fk_ctc_beam_search_lm: null pointer (LM tables / lm / total)");
  FK_CHECK_ARG(((uintptr_t)lm_table & 15) == 0, "fk_ctc_beam_search_lm: the hash table must be 16-byte aligned");
  FK_CHECK_ARG(lm_order >= 1 && lm_order <= 8, "fk_ctc_beam_search_lm: order = %lld outside 1 .. 8", (long long)lm_order);
  FK_CHECK_ARG(lm_cap >= 1 && lm_cap < (1LL << 31) && (lm_cap & (lm_cap - 1)) == 0, "fk_ctc_beam_search_lm: cap = %lld is no power of two below 2^31", (long long)lm_cap);
  FK_CHECK_ARG(lm_max_probe >= 1 && lm_max_probe <= lm_cap, "fk_ctc_beam_search_lm: max_probe = %lld outside 1 .. cap = %lld", (long long)lm_max_probe, (long long)lm_cap);
  FK_CHECK_ARG(lm_states >= 1 && lm_states < (1LL << 31) && lm_start_state >= 0 && lm_start_state < lm_states,
               "fk_ctc_beam_search_lm: states = %lld, start_state = %lld", (long long)lm_states, (long long)lm_start_state);
  FK_CHECK_ARG(C < (1LL << 31) - 1, "fk_ctc_beam_search_lm: C = %lld leaves no id for the end of sentence", (long long)C);
  FK_CHECK_ARG(std::isfinite(lm_weight) && std::isfinite(length_bonus), "fk_ctc_beam_search_lm: lm_weight = %g, length_bonus = %g must be finite",
               (double)lm_weight, (double)length_bonus);
  BeamLmArgs a;
  const int rc = beam_front("fk_ctc_beam_search_lm", logits, ldb, ldt, input_lengths, B, T, C, blank, W, K, nbest, pad, ids, ld_ids_b, ld_ids_h, lengths, am,
                            dtype, workspace, workspace_bytes, stream, a);
  if (rc != FK_OK) return rc;
  a.table = (const int4*)lm_table; a.bow = lm_bow; a.backoff = lm_backoff; a.uni_lp = lm_uni_lp; a.uni_next = lm_uni_next;
  a.lm_out = lm; a.total_out = total; a.lm_weight = lm_weight; a.length_bonus = length_bonus;
  a.S = (int)lm_states; a.cap_mask = (int)(lm_cap - 1); a.max_probe = (int)lm_max_probe; a.order = (int)lm_order;
  a.start_state = (int)lm_start_state; a.use_eos = use_eos != 0;
  FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_beam_kernel<TT, true>), dim3((unsigned)B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, a));
  FK_CHECK_LAUNCH("fk_ctc_beam_search_lm(recursion)");
  return FK_OK;
}

size_t fk_ctc_beam_lex_workspace_bytes(int64_t B, int64_t T, int64_t W, int64_t K) {
  const size_t base = fk_ctc_beam_workspace_bytes(B, T, W, K);
  return base ? base + a256((size_t)B * (T * W + 1) * sizeof(int)) : 0;
}

int fk_ctc_beam_search_lex(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t B, int64_t T, int64_t C, int64_t blank,
                           int64_t sep, int64_t W, int64_t K, int64_t nbest, int64_t pad, const int32_t* trie_table, int64_t trie_cap,
                           int64_t trie_max_probe, const int32_t* node_words, int64_t n_nodes, const int32_t* word_list, int64_t n_list, int64_t V,
                           const int32_t* lm_table, int64_t lm_cap, int64_t lm_max_probe, const float* lm_bow, const int32_t* lm_backoff,
                           int64_t lm_states, const float* lm_uni_lp, const int32_t* lm_uni_next, int64_t lm_start_state, int64_t lm_order,
                           float lm_weight, float word_bonus, int use_eos, int64_t* words, int64_t ld_words_b, int64_t ld_words_h,
                           int64_t* word_lengths, int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, int64_t* lengths, float* am, float* lm,
                           float* total, uint8_t* complete, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "fk_ctc_beam_search_lex";
  FK_CHECK_ARG(trie_table && node_words && word_list, "%s: null pointer (lexicon tables)", fn);
  FK_CHECK_ARG(lm_table && lm_bow && lm_backoff && lm_uni_lp && lm_uni_next, "%s: null pointer (word LM tables)", fn);
  FK_CHECK_ARG(words && word_lengths && lm && total && complete, "%s: null pointer (words / word_lengths / lm / total / complete)", fn);
  FK_CHECK_ARG(((uintptr_t)trie_table & 15) == 0 && ((uintptr_t)lm_table & 15) == 0, "%s: the hash tables must be 16-byte aligned", fn);
  FK_CHECK_ARG(((uintptr_t)node_words & 7) == 0, "%s: node_words must be 8-byte aligned", fn);
  if (const int rc = check_common(fn, dtype, logits && ids && lengths && am, B, T, C, blank)) return rc;
  FK_CHECK_ARG(sep >= 0 && sep < C && sep != blank, "%s: sep = %lld outside [0, C = %lld) or equal to blank = %lld", fn, (long long)sep, (long long)C,
               (long long)blank);
  FK_CHECK_ARG(trie_cap >= 1 && trie_cap < (1LL << 31) && (trie_cap & (trie_cap - 1)) == 0, "%s: trie cap = %lld is no power of two below 2^31", fn,
               (long long)trie_cap);
  FK_CHECK_ARG(trie_max_probe >= 1 && trie_max_probe <= trie_cap, "%s: trie max_probe = %lld outside 1 .. cap = %lld", fn, (long long)trie_max_probe,
               (long long)trie_cap);
  FK_CHECK_ARG(n_nodes >= 1 && n_nodes < (1LL << 31), "%s: nodes = %lld (the root is node 0)", fn, (long long)n_nodes);
  FK_CHECK_ARG(n_list >= 1 && n_list < (1LL << 31) && V >= 1 && V < (1LL << 31) - 1, "%s: word list of %lld entries, V = %lld words", fn, (long long)n_list,
               (long long)V);
  FK_CHECK_ARG(lm_order >= 1 && lm_order <= 8, "%s: order = %lld outside 1 .. 8", fn, (long long)lm_order);
  FK_CHECK_ARG(lm_cap >= 1 && lm_cap < (1LL << 31) && (lm_cap & (lm_cap - 1)) == 0, "%s: LM cap = %lld is no power of two below 2^31", fn, (long long)lm_cap);
  FK_CHECK_ARG(lm_max_probe >= 1 && lm_max_probe <= lm_cap, "%s: LM max_probe = %lld outside 1 .. cap = %lld", fn, (long long)lm_max_probe, (long long)lm_cap);
  FK_CHECK_ARG(lm_states >= 1 && lm_states < (1LL << 31) && lm_start_state >= 0 && lm_start_state < lm_states, "%s: states = %lld, start_state = %lld", fn,
               (long long)lm_states, (long long)lm_start_state);
  FK_CHECK_ARG(std::isfinite(lm_weight) && std::isfinite(word_bonus), "%s: lm_weight = %g, word_bonus = %g must be finite", fn, (double)lm_weight,
               (double)word_bonus);
  const int64_t Lw = T > 0 ? (T + 1) / 2 : 0;
  FK_CHECK_ARG(T <= 0 || (ld_words_h >= Lw && ld_words_b >= (nbest - 1) * ld_words_h + Lw), "%s: words strides %lld / %lld below [nbest = %lld, (T + 1) / 2 = %lld]",
               fn, (long long)ld_words_b, (long long)ld_words_h, (long long)nbest, (long long)Lw);
  const size_t need = fk_ctc_beam_lex_workspace_bytes(B, T, W, K);
  FK_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need), "%s: workspace too small (%zu bytes, fk_ctc_beam_lex_workspace_bytes gives %zu)", fn,
               workspace_bytes, need);
  BeamLexArgs a;
  const int rc = beam_front(fn, logits, ldb, ldt, input_lengths, B, T, C, blank, W, K, nbest, pad, ids, ld_ids_b, ld_ids_h, lengths, am, dtype, workspace,
                            workspace_bytes, stream, a);
  if (rc != FK_OK) return rc;
  a.table = (const int4*)lm_table; a.bow = lm_bow; a.backoff = lm_backoff; a.uni_lp = lm_uni_lp; a.uni_next = lm_uni_next;
  a.lm_out = lm; a.total_out = total; a.lm_weight = lm_weight; a.length_bonus = word_bonus;
  a.S = (int)lm_states; a.cap_mask = (int)(lm_cap - 1); a.max_probe = (int)lm_max_probe; a.order = (int)lm_order;
  a.start_state = (int)lm_start_state; a.use_eos = use_eos != 0;
  a.trie = (const int4*)trie_table; a.node_words = (const int2*)node_words; a.word_list = word_list;
  a.nword = (int*)((char*)workspace + fk_ctc_beam_workspace_bytes(B, T, W, K));
  a.words = words; a.ld_words_b = ld_words_b; a.ld_words_h = ld_words_h; a.word_lengths = word_lengths; a.complete = complete;
  a.sep = (int)sep; a.V = (int)V; a.n_nodes = (int)n_nodes; a.n_list = (int)n_list; a.tcap_mask = (int)(trie_cap - 1);
  a.tmax_probe = (int)trie_max_probe; a.Lw = (int)Lw;
  FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_beam_kernel<TT, true, true>), dim3((unsigned)B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, a));
  FK_CHECK_LAUNCH("fk_ctc_beam_search_lex(recursion)");
  return FK_OK;
}

int fk_ctc_prefix_init(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t S, int64_t T, int64_t C, int64_t blank,
                       int64_t W, const int64_t* prompt, int64_t prompt_ld, int64_t P, float* row_lse, float* state0, float* psi, int32_t* last,
                       int dtype, void* stream) {
  if (const int rc = prefix_check("fk_ctc_prefix_init", dtype, logits && row_lse && state0 && psi && last, ldb, ldt, S, T, C, blank, W)) return rc;
  FK_CHECK_ARG(P >= 0 && P <= PFX_MAX_PROMPT && (P == 0 || (prompt && prompt_ld >= P)), "fk_ctc_prefix_init: %lld prompt labels (at most %d; stride %lld)",
               (long long)P, PFX_MAX_PROMPT, (long long)prompt_ld);
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = S * T;
  CTC_LAUNCH_ROWS(ctc_row_lse_kernel, dtype, rows, C, s, (const TT*)logits, ldb, ldt, row_lse, rows, (int)T, (int)C);
  FK_CHECK_LAUNCH("fk_ctc_prefix_init(row_lse)");
  PfxInitArgs a;
  a.logits = logits; a.ldb = ldb; a.ldt = ldt; a.input_lengths = input_lengths; a.row_lse = row_lse; a.prompt = prompt; a.prompt_ld = prompt_ld;
  a.st0 = state0; a.psi = psi; a.last = last;
  a.T = (int)T; a.C = (int)C; a.blank = (int)blank; a.W = (int)W; a.P = (int)P;
  FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_prefix_init_kernel<TT>), dim3((unsigned)S), dim3(64), 0, s, a));
  FK_CHECK_LAUNCH("fk_ctc_prefix_init(state)");
  return FK_OK;
}

int fk_ctc_prefix_score(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, const float* row_lse, int64_t S, int64_t T,
                        int64_t C, int64_t blank, int64_t W, int64_t k, float* top_lp, const int64_t* top_id, int broadcast, float weight,
                        int64_t eos, const int32_t* fin, const int64_t* step, const int32_t* parent_log, const int64_t* tok_log, int64_t log_rows,
                        float* state0, float* state1, float* psi, int32_t* last, int dtype, void* stream) {
  if (const int rc = prefix_check("fk_ctc_prefix_score", dtype,
                                  logits && row_lse && top_lp && top_id && step && parent_log && tok_log && state0 && state1 && psi && last, ldb, ldt, S,
                                  T, C, blank, W))
    return rc;
  FK_CHECK_ARG(k >= 1 && k <= PFX_MAX_K, "fk_ctc_prefix_score: k = %lld outside the envelope (1 .. %d candidates, one wave)", (long long)k, PFX_MAX_K);
  FK_CHECK_ARG(weight >= 0.0f && weight <= 1.0f, "fk_ctc_prefix_score: weight = %g outside [0, 1]", (double)weight);
  FK_CHECK_ARG(log_rows >= 1 && state0 != state1, "fk_ctc_prefix_score: log_rows = %lld, or one buffer for both states", (long long)log_rows);
  FK_CHECK_ARG(eos < 0 || fin, "fk_ctc_prefix_score: an end-of-text id needs the finished flags");
  PfxArgs a;
  a.logits = logits; a.ldb = ldb; a.ldt = ldt; a.input_lengths = input_lengths; a.row_lse = row_lse; a.top_lp = top_lp; a.top_id = top_id;
  a.fin = fin; a.step = step; a.parent_log = parent_log; a.tok_log = tok_log; a.st[0] = state0; a.st[1] = state1; a.psi = psi; a.last = last;
  a.eos = eos; a.log_rows = log_rows; a.weight = weight;
  a.S = (int)S; a.T = (int)T; a.C = (int)C; a.blank = (int)blank; a.W = (int)W; a.k = (int)k; a.broadcast = broadcast != 0;
  const dim3 grid((unsigned)(broadcast ? S : S * W));
  FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_prefix_score_kernel<TT>), grid, dim3(64), 0, (hipStream_t)stream, a));
  FK_CHECK_LAUNCH("fk_ctc_prefix_score");
  return FK_OK;
}

}  // extern "C"
