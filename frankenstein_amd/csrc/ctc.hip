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
//   fk_ctc_collapse  greedy decoding behind fk_argmax_rows: merge repeated frames, drop blanks, ordered compaction by ballot + prefix count
//
// Device-side clamps (every access stays inside the buffers whatever the integers say): input_length into [0, T], target_length into
// [0, Lmax], a label into [0, C) and off the blank (a label equal to the blank becomes blank - 1, or 1 when the blank is 0).  With a
// clamped label the loss is meaningless but defined.
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
template <bool BLOCK> FK_DEV float group_max(float v, float* sh) {
  v = wave_max(v);
  if constexpr (BLOCK) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = -INFINITY;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) v = fmaxf(v, sh[i]);
  }
  return v;
}
template <bool BLOCK> FK_DEV float group_sum(float v, float* sh) {
  v = wave_sum(v);
  if constexpr (BLOCK) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0.0f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) v += sh[i];
  }
  return v;
}
FK_DEV int block_min_int(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) v = min(v, sh[i]);
  return v;
}

// Row sweep on the shared vector I/O: scalar elements up to the row's first 16-byte boundary, whole vectors, a scalar tail.  Any row
// stride and any C take the vector body (C = 50258 in fp32 leaves every other row 8 bytes off the boundary).
template <typename T> FK_DEV int row_head(const T* p, int C) {
  constexpr int N = VecIO<T>::N;
  const int h = (int)((N - (int)(((uintptr_t)p / sizeof(T)) % N)) % N);
  return h < C ? h : C;
}

// ---- launch 1: row_lse -------------------------------------------------------------------------------------------------------
// running (max, sum of exponentials) per lane, rescaled once per vector; exp(-inf - -inf) is never formed
FK_DEV void lse_push(float& m, float& s, float x) {
  const float mn = fmaxf(m, x);
  if (mn > -INFINITY) { s = s * __expf(m - mn) + __expf(x - mn); m = mn; }
}
template <typename T, bool BLOCK>
__global__ __launch_bounds__(256) void ctc_row_lse_kernel(const T* logits, int64_t ldb, int64_t ldt, float* row_lse, int64_t rows, int T_, int C) {
  constexpr int N = VecIO<T>::N, G = BLOCK ? 256 : 64, RPB = BLOCK ? 1 : 4;
  __shared__ float sh[8];
  const int gl = BLOCK ? threadIdx.x : (threadIdx.x & 63), sub = BLOCK ? 0 : (threadIdx.x >> 6);
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < rows; base += (int64_t)gridDim.x * RPB) {   // block-uniform trip count
    const int64_t row = base + sub;
    float m = -INFINITY, s = 0.0f;
    if (row < rows) {
      const T* lr = logits + (row / T_) * ldb + (row % T_) * ldt;
      const int head = row_head<T>(lr, C), nvec = (C - head) / N;
      for (int c = gl; c < head; c += G) lse_push(m, s, to_f32<T>(lr[c]));
      for (int i = gl; i < nvec; i += G) {
        float v[N];
        VecIO<T>::load(lr + head + i * N, v);
        float vm = m;
#pragma unroll
        for (int e = 0; e < N; ++e) vm = fmaxf(vm, v[e]);
        if (vm > -INFINITY) {
          float acc = s * __expf(m - vm);
#pragma unroll
          for (int e = 0; e < N; ++e) acc += __expf(v[e] - vm);
          s = acc;
          m = vm;
        }
      }
      for (int c = head + nvec * N + gl; c < C; c += G) lse_push(m, s, to_f32<T>(lr[c]));
    }
    const float M = group_max<BLOCK>(m, sh);
    const float tot = group_sum<BLOCK>(m > -INFINITY ? s * __expf(m - M) : 0.0f, sh);
    if (row < rows && gl == 0) row_lse[row] = M + logf(tot);
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
  int Tb = a.T;
  if (a.input_lengths) {
    const int64_t v = a.input_lengths[b];
    Tb = v < 0 ? 0 : (v > a.T ? a.T : (int)v);
  }
  const int64_t* tg = a.targets + (int64_t)b * a.ldtgt;
  int Lb;
  if (a.target_lengths) {
    const int64_t v = a.target_lengths[b];
    Lb = v < 0 ? 0 : (v > a.Lmax ? a.Lmax : (int)v);
  } else {
    int f = a.Lmax;
    for (int i = s; i < a.Lmax; i += blockDim.x)
      if (tg[i] == a.pad_value) { f = i; break; }
    Lb = block_min_int(f, sh_red);
  }
  const int S = 2 * Lb + 1;

  // the class of this thread's state
  int lab = a.blank;
  if ((s & 1) && (s >> 1) < Lb) {
    int64_t l = tg[s >> 1];
    l = l < 0 ? 0 : (l >= a.C ? a.C - 1 : l);
    if (l == a.blank) l = a.blank == 0 ? 1 : a.blank - 1;
    lab = (int)l;
  }
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
  const bool skip = live && odd && far >= 1 && far < S && sh_lab[far >= 0 && far < CTC_MAX_THREADS ? far : s] != lab;
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
  constexpr int N = VecIO<T>::N, G = BLOCK ? 256 : 64, RPB = BLOCK ? 1 : 4;
  __shared__ float sh[8];
  const int gl = BLOCK ? threadIdx.x : (threadIdx.x & 63), sub = BLOCK ? 0 : (threadIdx.x >> 6);
  const int64_t rows = (int64_t)a.B * a.T;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < rows; base += (int64_t)gridDim.x * RPB) {   // block-uniform trip count
    const int64_t row = base + sub;
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
      const int hl = row_head<T>(lr, a.C), hd = row_head<T>(dr, a.C);
      const int head = hl == hd ? hl : a.C, nvec = (a.C - head) / N;      // rows that disagree about the boundary go element by element
      for (int c = gl; c < head; c += G) dr[c] = from_f32<T>(full ? g * __expf(to_f32<T>(lr[c]) - lse) : fill);
      for (int i = gl; i < nvec; i += G) {
        float v[N], o[N];
        if (full) VecIO<T>::load(lr + head + i * N, v);
#pragma unroll
        for (int e = 0; e < N; ++e) o[e] = full ? g * __expf(v[e] - lse) : fill;
        VecIO<T>::store(dr + head + i * N, o);
      }
      for (int c = head + nvec * N + gl; c < a.C; c += G) dr[c] = from_f32<T>(full ? g * __expf(to_f32<T>(lr[c]) - lse) : fill);
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
  int Tb = T;
  if (input_lengths) {
    const int64_t v = input_lengths[b];
    Tb = v < 0 ? 0 : (v > T ? T : (int)v);
  }
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
  FK_DT_CHECK("fk_ctc_loss_fwd");
  FK_CHECK_ARG(logits && nll && loss2 && row_lse && workspace && (targets || Lmax == 0), "fk_ctc_loss_fwd: null pointer");
  FK_CHECK_ARG(B > 0 && T > 0 && B * T < (1LL << 31), "fk_ctc_loss_fwd: B = %lld, T = %lld", (long long)B, (long long)T);
  FK_CHECK_ARG(C >= 2 && C < (1LL << 31), "fk_ctc_loss_fwd: C = %lld, must be >= 2 (a class beside the blank)", (long long)C);
  FK_CHECK_ARG(blank >= 0 && blank < C, "fk_ctc_loss_fwd: blank = %lld outside [0, C = %lld)", (long long)blank, (long long)C);
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
  if (C > 1024)
    FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_row_lse_kernel<TT, true>), dim3((unsigned)(rows < 8192 ? rows : 8192)), dim3(256), 0, s, (const TT*)logits, ldb, ldt, row_lse, rows, (int)T, (int)C));
  else
    FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_row_lse_kernel<TT, false>), dim3((unsigned)(fk_cdiv(rows, 4) < 8192 ? fk_cdiv(rows, 4) : 8192)), dim3(256), 0, s, (const TT*)logits, ldb, ldt, row_lse, rows, (int)T, (int)C));
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
  FK_DT_CHECK("fk_ctc_loss_bwd");
  FK_CHECK_ARG(logits && row_lse && grad_out && dlogits && workspace, "fk_ctc_loss_bwd: null pointer");
  FK_CHECK_ARG(B > 0 && T > 0 && B * T < (1LL << 31), "fk_ctc_loss_bwd: B = %lld, T = %lld", (long long)B, (long long)T);
  FK_CHECK_ARG(C >= 2 && C < (1LL << 31), "fk_ctc_loss_bwd: C = %lld, must be >= 2 (a class beside the blank)", (long long)C);
  FK_CHECK_ARG(blank >= 0 && blank < C, "fk_ctc_loss_bwd: blank = %lld outside [0, C = %lld)", (long long)blank, (long long)C);
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
  if (C > 1024)
    FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_bwd_kernel<TT, true>), dim3((unsigned)(rows < 8192 ? rows : 8192)), dim3(256), 0, s, a));
  else
    FK_BY_DTYPE(dtype, TT, hipLaunchKernelGGL((ctc_bwd_kernel<TT, false>), dim3((unsigned)(fk_cdiv(rows, 4) < 8192 ? fk_cdiv(rows, 4) : 8192)), dim3(256), 0, s, a));
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

}  // extern "C"
