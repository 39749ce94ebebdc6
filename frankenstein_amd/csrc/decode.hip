// decode.hip — single-token decode step with the position on the DEVICE, so that one captured hipGraph replays for every new
// token (the reference re-runs the whole sequence per token, models/gpt2_model.py:336-340).
//   fk_gpt_embed_step  x[b, :] = wte[idx[b], :] + wpe[*pos, :]                               (models/gpt2_model.py:183-196, t = 1)
//   fk_kv_append       kv[b, *pos, :] = qkv[b, d : 3d]   (key | value rows of the new token into the per-layer cache)
//   fk_attn_decode     o[b, h, :] = softmax_j( q[b,h,:] . k[b,j,h,:] * scale ) v[b,j,h,:],  j = 0 .. *pos   (causal, one query)
// All three read the position from a device int32 (bumped by the host graph between steps).  HBM / latency-bound, no MFMA.
//   fk_sample_topk     the sampling tail of GPT.generate as one launch
//   fk_attn_decode_beam / fk_beam_topk / fk_beam_select    the step of the beam search on shared caches (ancestry table), further down
//   fk_attn_decode_beam_grouped / fk_beam_select_grouped   the same step for S sentences x W beams at once: rows g * W + b, a table of
//                       LOCAL slots, fk_kv_append folded into the attention launch, one select block per sentence + a ticket
//   fk_beam_select_eos / fk_beam_backtrack / fk_sample_topk_eos   end-of-text: finished beams and rows, length-normalised ranking, a live
//                       count for the host's early exit, and the walk through the logs on the device
//   fk_logit_rules      repetition penalty, n-gram ban and minimum length on the fp32 logits, in front of the sampling / fk_beam_topk launch;
//                       it keeps the token history of every row on the device (two buffers swapped by step parity under a beam search)
// The select, the beam attention and the sampling are one kernel template each, and so are their host sides (beam_select,
// check_ / launch_attn_decode_beam and sample_topk behind the kernels): the entry points of a family share their checks and their launch.
// What the kernels share is written once, in front of its first user:
//   clamp_index                       every slot / parent / table / token index that a corrupt input must not take outside its buffer
//   softmax_merge                     the online softmax of both attention kernels: the merge of the lanes' (m, l, o[]) across the wave
//                                     (wave_max / wave_sum of fk_common.h) and the four waves, and the store
//   row_key / for_row_keys            logit i of a row as the sampler and the beam top-k see it (scaled, with its sortable image), and the
//                                     strided or contiguous loop over a row
//   radix_select + bin_walk           the four 8-bit passes of radix_select_kth (a count per key) and mass_select_tau (a mass per key)
//   block_reduce / block_scan_inclusive   over the SAMPLE_THREADS of a sampling or top-k block
//   step_tail                         the end of a decode step: live rows, ticket, the last block advances the counters
//   rank_desc                         rank among (value descending, index ascending) by counting
// and on the host FK_BY_HEAD_DIM (nests with FK_BY_DTYPE), check_logit_rows and make_eos_args.
#include "fk_common.h"

namespace {

// x as an index into n entries: a corrupt or out-of-range value reads or writes a wrong entry, never outside the buffer
template <typename I> FK_DEV I clamp_index(I x, I n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }

template <typename T>
__global__ void gpt_embed_step_kernel(const int64_t* idx, const float* wte, const float* wpe, const int32_t* pos, T* out, int dim, int64_t vocab) {
  const int b = blockIdx.x;
  const int64_t tok = clamp_index(idx[b], vocab);
  const float* e = wte + tok * dim;
  const float* pe = wpe + (int64_t)pos[0] * dim;
  for (int c = threadIdx.x; c < dim; c += blockDim.x) out[(int64_t)b * dim + c] = from_f32<T>(e[c] + pe[c]);
}

template <typename T>
__global__ void kv_append_kernel(const T* qkv, T* kv, const int32_t* pos, int d, int64_t tmax) {
  const int b = blockIdx.x;
  const T* src = qkv + (int64_t)b * 3 * d + d;
  T* dst = kv + ((int64_t)b * tmax + pos[0]) * 2 * d;
  for (int c = threadIdx.x; c < 2 * d; c += blockDim.x) dst[c] = src[c];
}

// ---- online softmax of one query, shared by the two attention kernels.  A lane keeps (m, l, o[N]) over the keys it has seen: the running
// maximum of the scores, the sum of exp(s - m) and N elements of the values weighted so.  The update by one key stays written out in the two
// key loops: as a shared call it compiled, under -ffp-contract=fast, to the other fusion of o * a + pj * v in the fp32 beam kernels
// (profiles/decode_shared_asm_diff.txt), and the outputs are held to the bits of the loops as they stand.
// The merge of the partials of a block of 256 lanes, and the store of the D outputs to out[0 .. D).  The lanes of a wave whose numbers agree
// modulo STOP hold the same slice `sub` (N elements) of the D outputs: they are merged by shuffles (offsets 32 .. STOP), lanes 0 .. STOP - 1 of
// each wave put their slice into red[wave] (behind it the wave's maximum and sum), and thread t < D merges the four waves for output t.
// The order of the floating-point operations is part of the result: the weight w goes on before the shuffles, the division comes last.
template <typename T, int D, int N, int STOP> FK_DEV void softmax_merge(float m, float l, float (&o)[N], int sub, float (*red)[D + 2], T* out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float wm = wave_max<STOP>(m);
  const float w = (m == -INFINITY) ? 0.0f : __expf(m - wm);
  l = wave_sum<STOP>(l * w);
#pragma unroll
  for (int i = 0; i < N; ++i) o[i] = wave_sum<STOP>(o[i] * w);
  if (lane < STOP) {
    if (sub == 0) { red[wave][D] = wm; red[wave][D + 1] = l; }
#pragma unroll
    for (int i = 0; i < N; ++i) red[wave][sub * N + i] = o[i];
  }
  __syncthreads();
  if (tid < D) {
    const float M4 = fmaxf(fmaxf(red[0][D], red[1][D]), fmaxf(red[2][D], red[3][D]));
    float L = 0.0f, acc = 0.0f;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) {
      const float ww = (red[wv][D] == -INFINITY) ? 0.0f : __expf(red[wv][D] - M4);
      L += red[wv][D + 1] * ww;
      acc += red[wv][tid] * ww;
    }
    out[tid] = from_f32<T>(acc / L);
  }
}

// block = (b, h), 256 threads; thread t owns keys t, t + 256, ...; partial (max, sum, o[D]) merged wave- then block-wide
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_decode_kernel(const T* q, int64_t q_bs, const T* kv, int64_t kv_bs, int64_t kv_rs, T* out,
                                                          int64_t o_bs, const int32_t* pos, int H, float scale) {
  __shared__ float sq[D];
  __shared__ float red[4][D + 2];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int nk = pos[0] + 1;
  const int d_model = H * D;
  if (tid < D) sq[tid] = to_f32<T>(q[(int64_t)b * q_bs + h * D + tid]) * scale;
  __syncthreads();
  float m = -INFINITY, l = 0.0f, o[D];
#pragma unroll
  for (int i = 0; i < D; ++i) o[i] = 0.0f;
  for (int j = tid; j < nk; j += 256) {
    const T* kr = kv + (int64_t)b * kv_bs + (int64_t)j * kv_rs + h * D;
    const T* vr = kr + d_model;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < D; ++i) s += sq[i] * to_f32<T>(kr[i]);
    const float mn = fmaxf(m, s), a = __expf(m - mn), pj = __expf(s - mn);
    l = l * a + pj;
#pragma unroll
    for (int i = 0; i < D; ++i) o[i] = o[i] * a + pj * to_f32<T>(vr[i]);
    m = mn;
  }
  softmax_merge<T, D, D, 1>(m, l, o, 0, red, out + (int64_t)b * o_bs + h * D);      // every lane holds all of D
}

// ---- sampling tail of GPT.generate on the device (models/gpt2_model.py:340-351): logits / temperature -> top-k crop (everything below
// the k-th largest value becomes -inf; ties with it stay, like `logits < v[:, [-1]]`) -> softmax -> one multinomial draw.  One block per
// row; the k-th largest value by a 4-pass radix select over the order-preserving integer image of the fp32 logits; the draw by inverse
// CDF in index order with a Philox4x32-10 uniform keyed by (seed; step counter, row), so a captured graph draws fresh numbers on
// every replay: the LAST block to finish advances the device-side step counter (and the decode position) for the next replay.
constexpr int SAMPLE_THREADS = 1024;

FK_DEV unsigned f32_sortable(float x) {          // monotone: a < b  <=>  key(a) < key(b)   (-0 < +0, NaNs above +inf)
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// maximum (MAX) or sum of v over the SAMPLE_THREADS of the block; red: one word per wave
template <bool MAX> FK_DEV float block_reduce(float v, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  v = MAX ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  float r = MAX ? -INFINITY : 0.0f;
  for (int i = 0; i < SAMPLE_THREADS / 64; ++i) r = MAX ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

// Inclusive scan (Hillis-Steele) over the SAMPLE_THREADS words of LDS into which every thread has just stored its own
template <typename T> FK_DEV void block_scan_inclusive(T* scan) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int o = 1; o < SAMPLE_THREADS; o <<= 1) {
    const T add = tid >= o ? scan[tid - o] : T(0);
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
}

// Logit i of a row as the sampler and the beam top-k see it: x = row[i] * inv_temp and the sortable image of x
struct RowKey { float x; unsigned key; };
FK_DEV RowKey row_key(const float* row, int i, float inv_temp) {
  const float x = row[i] * inv_temp;
  return {x, f32_sortable(x)};
}
// f(i, x, key) for i = i0, i0 + stride, .. below i1: the block's strided pass over a row is (tid, V, SAMPLE_THREADS), a thread's contiguous chunk
// (i0, i1, 1).  The draw and the tie order depend on the chunk form; the loops that leave early or run backwards call row_key themselves.
template <typename F> FK_DEV void for_row_keys(const float* row, float inv_temp, int i0, int i1, int stride, F f) {
  for (int i = i0; i < i1; i += stride) {
    const RowKey e = row_key(row, i, inv_temp);
    f(i, e.x, e.key);
  }
}

// The first wave's walk over the 256 bins of a radix pass, from the top, until the running sum reaches the target rem0 = target(sum of all
// bins): lane l owns the bins 255 - 4l .. 252 - 4l, a scan finds the lane, and the lane walks its 4 bins and publishes the prefix with the
// bin's 8 bits in it and what of the target is left inside that bin.  CAN_MISS says what happens when the target lies beyond the total:
// without it bin 0 takes whatever is left, as a walk that stops at bin 1 would; with it no lane answers and *sel_rem stays as it is.
template <typename Acc, bool CAN_MISS, typename Target>
FK_DEV void bin_walk(const Acc* hist, unsigned prefix, int shift, unsigned* sel_prefix, Acc* sel_rem, Target target) {
  const int tid = threadIdx.x;                            // < 64
  Acc h[4], mine = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { h[q] = hist[255 - 4 * tid - q]; mine += h[q]; }
  Acc incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const Acc up = __shfl_up(incl, o, 64);
    if (tid >= o) incl += up;
  }
  const Acc rem0 = target(__shfl(incl, 63, 64));
  const Acc before = incl - mine;                         // what the bins above this lane's hold
  if (before < rem0 && (rem0 <= incl || (!CAN_MISS && tid == 63))) {      // one lane: the bins above hold less than the target, with its own they reach it
    Acc rem = rem0 - before;
    int q = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (q == c && h[c] < rem) { rem -= h[c]; q = c + 1; }
    }
    *sel_prefix = prefix | ((unsigned)(255 - 4 * tid - q) << shift);
    *sel_rem = rem;                                       // >= 1, and the chosen bin holds at least as much: the next pass reaches it too
  }
}

// A 4-pass radix select over the sortable keys of the V values row[i] * inv_temp, 8 bits per pass from the top: every pass adds weigh(x, key)
// (0: the key does not take part) of the keys that match the prefix found so far to a 256-bin histogram in LDS and walks the bins
// (bin_walk) for the one that holds the target; target(pass, total) names it, *sel_rem starts as rem_init.  Every thread of the block calls
// it and gets the same key; with CAN_MISS (rem_init is then 0) that is 0 when the first pass does not reach its target.  hist: 256 words of
// LDS, sel_prefix / sel_rem: one word each.
template <typename Acc, bool CAN_MISS, typename Weigh, typename Target>
FK_DEV unsigned radix_select(const float* row, int V, float inv_temp, Acc rem_init, Acc* hist, unsigned* sel_prefix, Acc* sel_rem, Weigh weigh, Target target) {
  const int tid = threadIdx.x;
  if (tid == 0) { *sel_prefix = 0u; *sel_rem = rem_init; }
#pragma unroll                                            // shift and mask are constants of each pass, and the first pass tests no prefix
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = *sel_prefix, mask_hi = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for_row_keys(row, inv_temp, tid, V, SAMPLE_THREADS, [&](int, float x, unsigned key) {
      if ((key & mask_hi) == prefix) {
        const Acc w = weigh(x, key);
        if (w) atomicAdd(&hist[(key >> shift) & 255u], w);
      }
    });
    __syncthreads();
    if (tid < 64) bin_walk<Acc, CAN_MISS>(hist, prefix, shift, sel_prefix, sel_rem, [&](Acc total) { return target(pass, total); });
    __syncthreads();
    if (CAN_MISS && pass == 0 && *sel_rem == 0) return 0u;      // block-uniform
  }
  return *sel_prefix;
}

// k-th largest of the V values row[i] * inv_temp (1 <= k <= V) as its sortable key: radix_select with a count of 1 per key and the target
// k, which the V >= k keys always reach (bin 0 takes whatever is left).  hist: 256 words of LDS, sel_prefix / sel_remaining: one word each.
// Behind it *sel_remaining says how many of the values EQUAL to the k-th belong to the k largest (k minus the count of strictly larger
// ones) and hist[key & 255] how many such values the row holds.
FK_DEV unsigned radix_select_kth(const float* row, int V, float inv_temp, int k, unsigned* hist, unsigned* sel_prefix, unsigned* sel_remaining) {
  return radix_select<unsigned, false>(row, V, inv_temp, (unsigned)k, hist, sel_prefix, sel_remaining, [](float, unsigned) { return 1u; },
                                       [&](int, unsigned) { return *sel_remaining; });
}

// Nucleus (top-p) threshold of fk_sample_topp: the smallest key v among the kept keys (>= kth) whose strictly larger kept keys hold less than
// top_p of the kept mass, mass(i) = exp(row[i] * inv_temp - mx).  radix_select with a histogram of MASS per bin instead of a count: the walk stops in the
// bin in which the running mass reaches the target.  The masses are summed as integers, floor(e * 2^32) <= 2^32 in 64-bit LDS words (V < 2^31
// of them cannot overflow), so neither the histogram nor any comparison depends on the order in which the atomics land.  The target is
// floor(top_p * total) + 1 units: key v stays iff mass_gt(v) <= floor(top_p * total), the rule `mass_gt < top_p * total` up to one unit of
// 2^-32.  A target beyond the total (top_p = 1 always, by construction) is not reached: 0 comes back and everything >= kth stays.
// Every thread of the block calls it and gets the same key.  mhist: 256 64-bit words of LDS, sel_prefix / sel_rem: one word each.
FK_DEV unsigned mass_select_tau(const float* row, int V, float inv_temp, unsigned kth, float mx, float top_p, unsigned long long* mhist, unsigned* sel_prefix,
                                unsigned long long* sel_rem) {
  return radix_select<unsigned long long, true>(
      row, V, inv_temp, 0ull, mhist, sel_prefix, sel_rem,
      [&](float x, unsigned key) {
        if (key < kth) return 0ull;
        const float e = __expf(x - mx);                     // <= 1: mx is the maximum of the kept values; NaN and 0 add nothing
        return e > 0.0f ? (unsigned long long)(e * 4294967296.0f) : 0ull;
      },
      [&](int pass, unsigned long long total) {
        if (pass != 0) return *sel_rem;
        // the first histogram holds every kept key: its sum is the total
        const unsigned long long rem0 = top_p >= 1.0f ? ~0ull : (unsigned long long)((double)top_p * (double)total) + 1ull;
        return rem0 > total ? 0ull : rem0;                  // not reached: no lane answers, *sel_rem stays 0 and 0 comes back
      });
}

// End-of-text state of the EOS variants below (all device pointers; unused and empty in the plain instantiations): fin[r] 0/1 (a finished
// beam, a done row), len[r] the generated tokens so far with the end-of-text token counted once, inv_lenpow[L] = 1 / L^alpha for
// L < n_lenpow (the kernels only multiply by it), live_acc the word the blocks add their unfinished rows to, live[0] what the last block
// found there.
struct EosArgs {
  int eos;
  int32_t* fin;
  int32_t* len;
  const float* inv_lenpow;
  int n_lenpow;
  unsigned* live_acc;
  int32_t* live;
};

// The end of a decode step, called by one thread of every block whose launch shares one step counter (and one position).  TICKET: the
// launch has gridDim.x blocks, every block takes a ticket behind its own writes and the last one, by when every block has read step[0]
// (and pos[0]) and has written its rows, clears the ticket and advances the counters; without it the launch is one block, which advances
// them itself.  EOS: every block first adds its unfinished rows to live_acc, and the last one fetches and clears the sum.  Only atomics
// carry a value between the blocks.
template <bool EOS, bool TICKET>
FK_DEV void step_tail(const EosArgs& ea, unsigned n_live, unsigned* ticket, int64_t* step, int64_t my_step, int32_t* pos_inc) {
  if constexpr (EOS) atomicAdd(ea.live_acc, n_live);
  if constexpr (TICKET) {
    __threadfence();
    if (atomicAdd(ticket, 1u) != gridDim.x - 1) return;
    if constexpr (EOS) {
      __threadfence();
      ea.live[0] = (int32_t)atomicExch(ea.live_acc, 0u);
    }
    ticket[0] = 0u;
  }
  step[0] = my_step + 1;
  if (pos_inc) pos_inc[0] += 1;
}

// EOS: a row with fin[b] != 0 draws nothing and emits ea.eos; a row that draws ea.eos becomes done; len[b] counts the tokens of a row up to
// and including its end-of-text token.  The draw of every other row is the plain kernel's (Philox keyed by step and row).
// NUCLEUS: behind the top-k crop a second threshold key, mass_select_tau; everything after the selection asks key >= max(kth, tau), and the
// Philox counter is the same, so top_p = 1 draws what the instantiation without it draws.  top_p is read by these instantiations only.
template <bool EOS, bool NUCLEUS>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_topk_kernel(const float* logits, int64_t ld, int V, float inv_temp, int top_k, float top_p,
                                                                     const unsigned long long* seed, int64_t* step, int32_t* pos_inc,
                                                                     int64_t* cur, int64_t* out, int64_t out_ld, int64_t out_cols, unsigned* ticket,
                                                                     EosArgs ea) {
  __shared__ unsigned hist[256];
  __shared__ float red[SAMPLE_THREADS / 64];
  __shared__ float scan[SAMPLE_THREADS];
  __shared__ unsigned sel_prefix, sel_remaining;
  __shared__ int winner;
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* row = logits + (int64_t)b * ld;
  const int64_t my_step = step[0];                       // read before anybody can advance it (the advance happens after the last block)
  if constexpr (EOS) {
    if (ea.eos >= 0 && ea.fin[b] != 0) {                 // block-uniform: no barrier is skipped by part of a block; without an id no row is done
      if (tid == 0) {
        cur[b] = ea.eos;
        if (out && my_step >= 0 && my_step < out_cols) out[(int64_t)b * out_ld + my_step] = ea.eos;
        step_tail<true, true>(ea, 0u, ticket, step, my_step, pos_inc);
      }
      return;
    }
  }

  // ---- k-th largest key (top_k <= 0 or >= V: keep everything)
  unsigned kth = 0u;
  if (top_k > 0 && top_k < V) kth = radix_select_kth(row, V, inv_temp, top_k, hist, &sel_prefix, &sel_remaining);
  // ---- softmax over the kept logits: maximum, then the sum of exp; per-thread partial sums of CONTIGUOUS index chunks for the draw
  float mx = -INFINITY;
  for_row_keys(row, inv_temp, tid, V, SAMPLE_THREADS, [&](int, float x, unsigned key) {
    if (key >= kth) mx = fmaxf(mx, x);
  });
  mx = block_reduce<true>(mx, red);
  if constexpr (NUCLEUS) {                                // the most likely token always stays, so mx is the nucleus's maximum as well
    __shared__ unsigned long long mhist[256];
    __shared__ unsigned long long sel_rem;
    const unsigned tau = mass_select_tau(row, V, inv_temp, kth, mx, top_p, mhist, &sel_prefix, &sel_rem);
    kth = max(kth, tau);
  }
  const int chunk = (V + SAMPLE_THREADS - 1) / SAMPLE_THREADS, i0 = tid * chunk, i1 = min(V, i0 + chunk);
  float part = 0.0f;
  for_row_keys(row, inv_temp, i0, i1, 1, [&](int, float x, unsigned key) {
    if (key >= kth) part += __expf(x - mx);
  });
  scan[tid] = part;
  block_scan_inclusive(scan);                             // of the chunk sums
  const float total = scan[SAMPLE_THREADS - 1];
  // ---- one uniform in [0, 1) and the first index whose cumulative mass exceeds u * total
  unsigned c[4] = {(unsigned)my_step, (unsigned)((unsigned long long)my_step >> 32), (unsigned)b, 0x5A3Cu};
  philox4x32_10((unsigned)seed[0], (unsigned)(seed[0] >> 32), c);
  const float target = (float)(c[0] >> 8) * (1.0f / 16777216.0f) * total;
  if (tid == 0) winner = -1;
  __syncthreads();
  const float before = tid == 0 ? 0.0f : scan[tid - 1];
  if (part > 0.0f && before <= target && target < scan[tid]) {
    float acc = before;
    int pick = -1;
    for (int i = i0; i < i1; ++i) {
      const RowKey rk = row_key(row, i, inv_temp);
      if (rk.key >= kth) {
        const float e = __expf(rk.x - mx);
        acc += e;
        if (e > 0.0f) pick = i;                           // last kept index WITH MASS seen: the fallback when rounding leaves acc <= target
        if (acc > target) break;
      }
    }
    winner = pick;
  }
  __syncthreads();
  if (tid == 0) {
    int w = winner;
    if (w < 0) {                                          // target >= total by rounding: the last kept index with mass (a -inf entry is kept by the
      for (int i = V - 1; i >= 0; --i) {                  // crop whenever top_k is off, and is never a token to emit)
        const RowKey rk = row_key(row, i, inv_temp);
        if (rk.key >= kth && __expf(rk.x - mx) > 0.0f) { w = i; break; }
      }
    }
    if (w < 0) {                                          // a row without any mass (all -inf, NaN): the last kept index, as ever
      for (int i = V - 1; i >= 0; --i)
        if (row_key(row, i, inv_temp).key >= kth) { w = i; break; }
    }
    cur[b] = w;
    unsigned n_live = 0u;
    if constexpr (EOS) {
      if (out && my_step >= 0 && my_step < out_cols) out[(int64_t)b * out_ld + my_step] = w;
      const bool ended = ea.eos >= 0 && w == ea.eos;
      ea.len[b] = (int32_t)((unsigned)ea.len[b] + 1u);
      if (ended) ea.fin[b] = 1;
      n_live = ended ? 0u : 1u;
    } else {
      if (out && my_step < out_cols) out[(int64_t)b * out_ld + my_step] = w;       // a step counter past the buffer is not a write past it
    }
    step_tail<EOS, true>(ea, n_live, ticket, step, my_step, pos_inc);
  }
}

// ---- rules that depend on the tokens already emitted (include/franken_hip.h, fk_logit_rules, has the rule).  One block per logits row, the
// threads stride over the row's history h[0 .. L), L = t0 + *step, which this launch first brings up to date and copies into LDS:
//   plain (hist_b == NULL): the row's buffer gets cur[r] at column L - 1 (step > 0);
//   beam: the buffers swap by the parity of the step: new[r, :L-1] = old[g * W + clamp(parent_log[step - 1, r]), :L-1], new[r, L-1] = cur[r],
//         so no block reads what another block of the launch writes; `broadcast` (the first step: one logits row per sentence) reads row g * W
//         and appends nothing.
// Then read-all, barrier, write-all: every history position loads the logit of its token, the block meets, and the penalised values are
// stored, so a token that occurs several times is penalised once and its occurrences store the same value; behind a second barrier the
// bans store -inf, which therefore win over the penalty.  A step counter that is negative, past the history buffer or (beam) past the logs
// leaves the launch without any write.
constexpr int RULES_THREADS = 256, RULES_MAX_HIST = 4096;

__global__ __launch_bounds__(RULES_THREADS) void logit_rules_kernel(float* logits, int64_t ld, int V, float p, float inv_p, int n, int m, int eos, const int64_t* step,
                                                                    const int64_t* cur, int32_t* hist_a, int32_t* hist_b, int64_t hist_ld, int t0,
                                                                    const int32_t* parent_log, int64_t log_rows, int W, int broadcast) {
  __shared__ int32_t h[RULES_MAX_HIST];
  __shared__ float zs[RULES_MAX_HIST];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int64_t s = step[0];
  const bool beam = hist_b != nullptr;
  if (s < 0 || (int64_t)t0 + s > hist_ld || (int64_t)t0 + s > RULES_MAX_HIST || (beam && s > log_rows)) return;      // block-uniform
  const int L = t0 + (int)s;
  const int32_t* src;
  int32_t* dst;
  bool append = s > 0;
  if (!beam) {
    src = dst = hist_a + (int64_t)r * hist_ld;
  } else {
    int32_t* nw = (s & 1) ? hist_b : hist_a;
    int32_t* od = (s & 1) ? hist_a : hist_b;
    if (broadcast) {
      src = dst = nw + (int64_t)r * W * hist_ld;
      append = false;
    } else if (!append) {
      src = dst = nw + (int64_t)r * hist_ld;
    } else {
      const int pr = clamp_index(parent_log[(s - 1) * (int64_t)gridDim.x + r], W);      // a corrupt log reads a wrong row of its own sentence
      src = od + (int64_t)((r / W) * W + pr) * hist_ld;
      dst = nw + (int64_t)r * hist_ld;
    }
  }
  for (int j = tid; j < L; j += RULES_THREADS) {
    int32_t v;
    if (append && j == L - 1) {
      const int64_t c = cur[r];
      v = (c < 0 || c >= V) ? -1 : (int32_t)c;
      dst[j] = v;
    } else {
      v = src[j];
      if (dst != src) dst[j] = v;
    }
    h[j] = v;
  }
  __syncthreads();
  float* z = logits + (int64_t)r * ld;
  if (p != 1.0f) {                                        // block-uniform
    for (int j = tid; j < L; j += RULES_THREADS) {
      const int v = h[j];
      if (v >= 0 && v < V && v != eos) zs[j] = z[v];
    }
    __syncthreads();
    for (int j = tid; j < L; j += RULES_THREADS) {
      const int v = h[j];
      if (v >= 0 && v < V && v != eos) {
        const float x = zs[j];
        z[v] = x > 0.0f ? x * inv_p : x * p;              // one fp32 multiply: the host restatement agrees bit for bit
      }
    }
    __syncthreads();
  }
  if (n >= 1 && L >= n) {
    const int32_t* tail = h + (L - n + 1);                // the last n - 1 tokens
    for (int i = n - 1 + tid; i < L; i += RULES_THREADS) {
      const int v = h[i];
      if (v < 0 || v >= V || v == eos) continue;
      bool match = true;
      for (int c = 0; c < n - 1; ++c) match = match && h[i - n + 1 + c] == tail[c];
      if (match) z[v] = -INFINITY;
    }
  }
  if (tid == 0 && eos >= 0 && eos < V && s < (int64_t)m) z[eos] = -INFINITY;
}

// ---- beam search on the caches (models/gpt2_model.py:355-416).  The W beams share ONE set of caches [W, Tmax, 2d]: slot b holds the rows
// that beam position b wrote, and the ancestry table anc[b, j] names the slot in which beam b's row j lives, so reordering the beams
// rewrites W x (pos + 1) int32 and never moves a key or a value.

// block = (h, b), 256 threads.  A key row of D elements is spread over LPK = D / (16 bytes of T) neighbouring lanes, one 16-byte load
// each, so a wave reads 64 / LPK whole rows per trip as contiguous 16-byte pieces; the score is summed across the LPK lanes, every
// lane keeps the running (max, sum) of its key group and its own 16-byte slice of the output, and the groups are merged across the
// wave (lanes with the same slice) and then across the four waves.
//
// GROUPED: the rows are S sentences x W beams, row b = g * W + beam, and the table holds LOCAL slots: row j < pos of row b lives in slot
// g * W + clamp(anc[b, j], 0, W - 1), so a corrupt entry stays inside its own sentence.  tmax (rows of a cache slot, > 0) bounds the
// position: *pos >= tmax (or >= anc_ld) counts as the last row, never a read or a write outside the cache.  append != 0 folds fk_kv_append
// into the launch: q is then the whole [q | k | v] row, and the LPK lanes that own key *pos load head h's slices of k and v from it,
// store them to kv[b, *pos] and use them from their registers, so no lane reads what another lane or another block wrote.
template <typename T, int D, bool GROUPED>
__global__ __launch_bounds__(256) void attn_decode_beam_kernel(const T* q, int64_t q_bs, T* kv, int64_t kv_bs, int64_t kv_rs, int tmax, const int32_t* anc,
                                                               int64_t anc_ld, T* out, int64_t o_bs, const int32_t* pos, int W, int H, float scale,
                                                               int append) {
  constexpr int VN = VecIO<T>::N, LPK = D / VN, GROUPS = 256 / LPK;
  typedef T vec_t __attribute__((ext_vector_type(VN)));
  __shared__ float red[4][D + 2];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int sub = tid % LPK, grp = tid / LPK;
  int p = pos[0];
  int base = 0;                                           // first slot of this row's sentence
  if constexpr (GROUPED) {
    base = (b / W) * W;
    const int last = (int)(anc_ld < (int64_t)tmax ? anc_ld : (int64_t)tmax) - 1;
    p = p > last ? last : p;
  }
  const int nk = p + 1;
  const int d_model = H * D;
  float qf[VN], o[VN];
#pragma unroll
  for (int i = 0; i < VN; ++i) {
    qf[i] = to_f32<T>(q[(int64_t)b * q_bs + h * D + sub * VN + i]) * scale;
    o[i] = 0.0f;
  }
  float m = -INFINITY, l = 0.0f;
  const int32_t* arow = anc + (int64_t)b * anc_ld;
  for (int j = grp; j < nk; j += GROUPS) {
    int slot = b - base;                                  // the newest row is the beam's own (fk_kv_append has just written it, or this launch does)
    if (j < p) {
      slot = clamp_index(arow[j], W);                     // a corrupt table reads a wrong row, never outside the cache
    }
    T* kr = kv + (int64_t)(base + slot) * kv_bs + (int64_t)j * kv_rs + h * D + sub * VN;
    vec_t kvec, vvec;
    if (GROUPED && append && j == p) {                    // slot == b - base here: the row is this block's own
      const T* nr = q + (int64_t)b * q_bs + d_model + h * D + sub * VN;
      kvec = *reinterpret_cast<const vec_t*>(nr);
      vvec = *reinterpret_cast<const vec_t*>(nr + d_model);
      *reinterpret_cast<vec_t*>(kr) = kvec;
      *reinterpret_cast<vec_t*>(kr + d_model) = vvec;
    } else {
      kvec = *reinterpret_cast<const vec_t*>(kr);
      vvec = *reinterpret_cast<const vec_t*>(kr + d_model);
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < VN; ++i) s += qf[i] * to_f32<T>(kvec[i]);
#pragma unroll
    for (int off = LPK >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mn = fmaxf(m, s), a = __expf(m - mn), pj = __expf(s - mn);
    l = l * a + pj;
#pragma unroll
    for (int i = 0; i < VN; ++i) o[i] = o[i] * a + pj * to_f32<T>(vvec[i]);
    m = mn;
  }
  // the key groups of a wave are the lanes that hold the same slice of D
  softmax_merge<T, D, VN, LPK>(m, l, o, sub, red, out + (int64_t)b * o_bs + h * D);
}

// Rank of the entry (v, id) among the n entries (val[c], ids ? ids[c] : c) ordered by value descending, then id ascending: the count of
// the entries with valid(c) that come before it.  Ranks of distinct entries are distinct, whatever order the entries were stored in.
struct AllValid { FK_DEV bool operator()(int) const { return true; } };
template <typename T, typename Valid = AllValid> FK_DEV int rank_desc(const T* val, const int* ids, int n, T v, int id, Valid valid = Valid()) {
  int rank = 0;
  for (int c = 0; c < n; ++c) rank += (valid(c) && (val[c] > v || (val[c] == v && (ids ? ids[c] : c) < id))) ? 1 : 0;
  return rank;
}

// One block per row: lp = x - logsumexp(x), x = logits * (1 / temperature); the k largest lp, descending, equal values by ascending id.
// The k-th largest comes from the radix select above; everything strictly above it is collected in any order (LDS append) and what
// is still missing is taken from the values EQUAL to it by ascending id; a rank sort over (value, id) then fixes the output order, so
// nothing depends on the order in which the atomics landed.
constexpr int BEAM_MAX_K = 64, BEAM_MAX_W = 16;

__global__ __launch_bounds__(SAMPLE_THREADS) void beam_topk_kernel(const float* logits, int64_t ld, int V, float inv_temp, int k, float* top_lp,
                                                                   int64_t* top_id) {
  __shared__ unsigned hist[256];
  __shared__ float red[SAMPLE_THREADS / 64];
  __shared__ unsigned scan[SAMPLE_THREADS];
  __shared__ unsigned sel_prefix, sel_remaining, n_above;
  __shared__ unsigned ckey[BEAM_MAX_K];
  __shared__ int cid[BEAM_MAX_K];
  const int tid = threadIdx.x, r = blockIdx.x;
  const float* row = logits + (int64_t)r * ld;
  if (tid < BEAM_MAX_K) { ckey[tid] = 0u; cid[tid] = 0; }
  const unsigned kth = radix_select_kth(row, V, inv_temp, k, hist, &sel_prefix, &sel_remaining);
  const unsigned n_eq_take = sel_remaining, n_eq = hist[kth & 255u];        // ties with the k-th value: wanted, present
  const int n_gt = k - (int)n_eq_take;
  if (tid == 0) n_above = 0u;
  // ---- log-sum-exp over the whole row
  float mx = -INFINITY;
  for_row_keys(row, inv_temp, tid, V, SAMPLE_THREADS, [&](int, float x, unsigned) { mx = fmaxf(mx, x); });
  mx = block_reduce<true>(mx, red);
  float part = 0.0f;
  const bool take_all_eq = n_eq == n_eq_take;              // no tie straddles rank k: everything >= the k-th value is in
  for_row_keys(row, inv_temp, tid, V, SAMPLE_THREADS, [&](int i, float x, unsigned key) {
    part += expf(x - mx);
    if (key > kth || (take_all_eq && key == kth)) {
      const unsigned at = atomicAdd(&n_above, 1u);
      if (at < (unsigned)BEAM_MAX_K) { ckey[at] = key; cid[at] = i; }
    }
  });
  const float lse = mx + logf(block_reduce<false>(part, red));
  if (!take_all_eq) {                                      // block-uniform.  The first n_eq_take ids among the ties: contiguous chunks + a scan of their counts
    const int chunk = (V + SAMPLE_THREADS - 1) / SAMPLE_THREADS, i0 = (int)min((int64_t)V, (int64_t)tid * chunk), i1 = (int)min((int64_t)V, (int64_t)i0 + chunk);
    unsigned mine = 0u;
    for_row_keys(row, inv_temp, i0, i1, 1, [&](int, float, unsigned key) { mine += key == kth ? 1u : 0u; });
    scan[tid] = mine;
    block_scan_inclusive(scan);
    unsigned rank = scan[tid] - mine;                      // ties in front of this chunk
    for (int i = i0; i < i1 && rank < n_eq_take; ++i) {
      if (row_key(row, i, inv_temp).key == kth) {
        const unsigned at = (unsigned)n_gt + rank;
        if (at < (unsigned)BEAM_MAX_K) { ckey[at] = kth; cid[at] = i; }
        ++rank;
      }
    }
  }
  __syncthreads();
  if (tid < k) {
    const int mi = cid[tid];
    const int rank = rank_desc(ckey, cid, k, ckey[tid], mi);
    top_lp[(int64_t)r * k + rank] = row_key(row, mi, inv_temp).x - lse;
    top_id[(int64_t)r * k + rank] = mi;
  }
}

// One block: the draw, the selection and the bookkeeping of one beam-search step (models/gpt2_model.py:384-408).
constexpr int BEAM_SELECT_THREADS = 256;

//
// GROUPED: one block per sentence g = blockIdx.x of gridDim.x, each running the same step on ITS W beams: top_lp / top_id rows at
// g * group_stride + i * row_stride, scores / cur / the table rows g * W .., the logs [steps, S, W], the Philox key seed[g].  The table
// entries are local slots in [0, W), so the ancestry update is the one-sentence update on the rows of the sentence.  All blocks read the
// one step counter and the one position on entry; the last block to finish (ticket) advances them, as in sample_topk_kernel.
//
// EOS (with GROUPED): the end-of-text rules of fk_beam_select_eos.  A finished beam proposes ONE candidate, itself (token ea.eos, its score
// unchanged, its length unchanged); the candidates are ranked by norm = raw * inv_lenpow[clamp(L, 0, n_lenpow - 1)], one fp32 multiply
// behind the one fp32 add of raw, so a table of ones ranks by raw bit for bit; scores[] keeps the raw sums.
template <bool GROUPED, bool EOS>
__global__ __launch_bounds__(BEAM_SELECT_THREADS) void beam_select_kernel(const float* top_lp, const int64_t* top_id, int64_t row_stride, int64_t group_stride,
                                                                          int W, int k, float* scores, const unsigned long long* seed, int64_t* step,
                                                                          const int32_t* pos, int32_t* pos_inc, int64_t* cur, int32_t* parent_log,
                                                                          int64_t* tok_log, int64_t log_rows, int32_t* anc, int64_t anc_ld,
                                                                          unsigned* ticket, EosArgs ea) {
  __shared__ float gum[BEAM_MAX_W * BEAM_MAX_K];
  __shared__ float sc[BEAM_MAX_W], cand[BEAM_MAX_W * BEAM_MAX_W];
  __shared__ int pick[BEAM_MAX_W * BEAM_MAX_W], surv[BEAM_MAX_W], parent[BEAM_MAX_W];
  __shared__ float cnorm[BEAM_MAX_W * BEAM_MAX_W];       // EOS only, like the three below
  __shared__ int sfin[BEAM_MAX_W], slen[BEAM_MAX_W], alive[BEAM_MAX_W];
  const int tid = threadIdx.x;
  const int64_t my_step = step[0];                       // read before anybody can advance it (the advance happens after the last block)
  const int p = pos[0];
  int64_t log_ld = W;                                    // one row of the logs
  if constexpr (GROUPED) {
    const int g = blockIdx.x;
    top_lp += g * group_stride;
    top_id += g * group_stride;
    scores += g * W;
    cur += g * W;
    seed += g;
    anc += (int64_t)g * W * anc_ld;
    log_ld = (int64_t)gridDim.x * W;
    if (parent_log) { parent_log += g * W; tok_log += g * W; }
    if constexpr (EOS) { ea.fin += g * W; ea.len += g * W; }
  }
  const unsigned long long sd = seed[0];
  if (tid < W) { sc[tid] = scores[tid]; surv[tid] = 0; }
  if constexpr (EOS) {
    if (tid < W) { sfin[tid] = (ea.eos >= 0 && ea.fin[tid] != 0) ? 1 : 0; slen[tid] = ea.len[tid]; }   // without an id no beam is finished
  }
  if (tid < W * W) pick[tid] = 0;
  // ---- Gumbel keys: the W largest of lp + G draw W entries without replacement with probability ~ exp(lp)
  // two trips side by side would be packed into v_pk_*_f32 with op_sel half-swaps, which this library keeps out of its code
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int e = tid; e < W * k; e += BEAM_SELECT_THREADS) {
    const int i = e / k, j = e - i * k;
    unsigned c[4] = {(unsigned)my_step, (unsigned)((unsigned long long)my_step >> 32), (unsigned)i, 0xBEA30000u | (unsigned)j};
    philox4x32_10((unsigned)sd, (unsigned)(sd >> 32), c);
    const float u = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    gum[e] = top_lp[i * row_stride + j] - logf(-logf(u));
  }
  __syncthreads();
  for (int e = tid; e < W * k; e += BEAM_SELECT_THREADS) {            // draw rank of entry j inside beam i (ties: the lower j first)
    const int i = e / k, j = e - i * k;
    const int rank = rank_desc(gum + i * k, nullptr, k, gum[e], j);
    if (rank < W) pick[i * W + rank] = j;
  }
  __syncthreads();
  // ---- the W best of the W * W candidates: score descending, then parent, then draw rank (= candidate number ascending)
  const int nc = W * W;
  if constexpr (EOS) {
    if (tid < nc) {
      const int i = tid / W;
      const bool done = sfin[i] != 0;
      const float raw = done ? sc[i] : sc[i] + top_lp[i * row_stride + pick[tid]];
      const int L = done ? slen[i] : (int)((unsigned)slen[i] + 1u);
      cand[tid] = raw;
      cnorm[tid] = raw * ea.inv_lenpow[clamp_index(L, ea.n_lenpow)];              // a length past the table ranks with its last entry
    }
    __syncthreads();
    const auto valid = [&](int c) { return !(sfin[c / W] != 0 && c % W > 0); };   // a finished beam has its candidate 0 only; at least W candidates are valid
    if (tid < nc && valid(tid)) {
      const int rank = rank_desc(cnorm, nullptr, nc, cnorm[tid], tid, valid);
      if (rank < W) surv[rank] = tid;
    }
  } else {
    if (tid < nc) cand[tid] = sc[tid / W] + top_lp[(tid / W) * row_stride + pick[tid]];
    __syncthreads();
    if (tid < nc) {
      const int rank = rank_desc(cand, nullptr, nc, cand[tid], tid);
      if (rank < W) surv[rank] = tid;
    }
  }
  __syncthreads();
  if (tid < W) {
    const int c = surv[tid], pr = c / W;
    int64_t tok = top_id[pr * row_stride + pick[c]];
    if constexpr (EOS) {
      const bool done = sfin[pr] != 0;
      if (done) tok = ea.eos;
      const int ended = (done || (ea.eos >= 0 && tok == ea.eos)) ? 1 : 0;
      ea.len[tid] = done ? slen[pr] : (int)((unsigned)slen[pr] + 1u);
      ea.fin[tid] = ended;
      alive[tid] = 1 - ended;
    }
    parent[tid] = pr;
    scores[tid] = cand[c];
    cur[tid] = tok;
    if (my_step >= 0 && my_step < log_rows) {
      parent_log[my_step * log_ld + tid] = pr;
      tok_log[my_step * log_ld + tid] = tok;
    }
  }
  __syncthreads();
  // ---- ancestry: the new beam b continues beam parent[b]; one thread owns a column and reads all of it before it writes
  for (int64_t j = tid; j <= p && j < anc_ld; j += BEAM_SELECT_THREADS) {
    int old[BEAM_MAX_W];
#pragma unroll
    for (int x = 0; x < BEAM_MAX_W; ++x) old[x] = (x < W && j < p) ? anc[x * anc_ld + j] : x;
    for (int b = 0; b < W; ++b) {
      const int pr = parent[b];
      int v = old[0];
#pragma unroll
      for (int x = 1; x < BEAM_MAX_W; ++x) v = pr == x ? old[x] : v;
      anc[b * anc_ld + j] = v;
    }
  }
  if constexpr (GROUPED) __syncthreads();                  // the whole block has written its rows of the table
  if (tid == 0) {                                          // every read of the counters is behind a barrier above
    unsigned n_live = 0u;
    if constexpr (EOS) {
      for (int b = 0; b < W; ++b) n_live += (unsigned)alive[b];
    }
    step_tail<EOS, GROUPED>(ea, n_live, ticket, step, my_step, pos_inc);      // one block and no ticket unless GROUPED
  }
}

// The walk of the host through the logs, on the device: block g = one sentence, thread b < W = one final beam.  n = min(*step, log_rows)
// steps are on record; beam b's token of step t is tok_log[t, g, x_t] with x_{n-1} = b and x_{t-1} = clamp(parent_log[t, g, x_t], 0, W-1).
// The beams are ranked by scores * inv_lenpow[clamp(len)] descending, then by beam number, and beam b's row goes to out_ids[g, rank]:
// columns t0 .. t0+n-1 its tokens, the columns behind them `pad`; nothing left of t0 (the caller's prompt) and nothing right of out_cols.
constexpr int BACKTRACK_THREADS = 64;

__global__ __launch_bounds__(BACKTRACK_THREADS) void beam_backtrack_kernel(const int32_t* parent_log, const int64_t* tok_log, int64_t log_rows, int W,
                                                                           const int64_t* step, const float* scores, const int32_t* len,
                                                                           const float* inv_lenpow, int n_lenpow, int64_t* out_ids, int64_t out_ld,
                                                                           int64_t out_cols, int64_t t0, int64_t pad, float* out_scores, int32_t* out_len) {
  __shared__ float norm[BEAM_MAX_W];
  const int g = blockIdx.x, b = threadIdx.x;
  const int64_t log_ld = (int64_t)gridDim.x * W;
  int64_t n = step[0];
  n = n < 0 ? 0 : (n > log_rows ? log_rows : n);          // a counter past the logs is not a read past them
  float raw = 0.0f;
  int L = 0;
  if (b < W) {
    raw = scores[g * W + b];
    L = len[g * W + b];
    norm[b] = raw * inv_lenpow[clamp_index(L, n_lenpow)];
  }
  __syncthreads();
  if (b >= W) return;
  const int rank = rank_desc(norm, nullptr, W, norm[b], b);
  int64_t* row = out_ids + ((int64_t)g * W + rank) * out_ld;
  int x = b;
  for (int64_t t = n - 1; t >= 0; --t) {
    const int64_t at = t * log_ld + (int64_t)g * W + x;
    if (t0 + t < out_cols) row[t0 + t] = tok_log[at];
    x = clamp_index(parent_log[at], W);
  }
  for (int64_t c = t0 + n; c < out_cols; ++c) row[c] = pad;
  out_scores[g * W + rank] = raw;
  out_len[g * W + rank] = L;
}

}  // namespace

// What the entry points of a family share, written once: the argument checks, the launch and its check.  `fn` is the entry point's name, `ptrs`
// whether all the pointers it needs are there; each returns FK_OK or the fk_set_error code.

// Host head_dim dispatch: the statement(s) are compiled once per supported head_dim with `DD` a constant and the arm of `D` (checked by the
// caller: 16, 32, 64 or 128) runs.  Nests with FK_BY_DTYPE.
#define FK_BY_HEAD_DIM(D, DD, ...)                                \
  do {                                                            \
    if ((D) == 16) { constexpr int DD = 16; __VA_ARGS__; }        \
    else if ((D) == 32) { constexpr int DD = 32; __VA_ARGS__; }   \
    else if ((D) == 64) { constexpr int DD = 64; __VA_ARGS__; }   \
    else { constexpr int DD = 128; __VA_ARGS__; }                 \
  } while (0)

// `rows` rows of V logits, ld apart: one block per row (grid x), 32-bit indices inside a row
static int check_logit_rows(const char* fn, int64_t rows, int64_t V, int64_t ld) {
  FK_CHECK_ARG(rows > 0 && rows < 65536 && V > 0 && V < (1LL << 31) && ld >= V, "%s: bad arguments (rows=%lld V=%lld ld=%lld)", fn, (long long)rows, (long long)V,
               (long long)ld);
  return FK_OK;
}

// The end-of-text state of a launch from the entry point's arguments: an id of 2^31 or more is refused, a negative one means "none" (-1)
static int make_eos_args(const char* fn, int64_t eos, int32_t* fin, int32_t* len, const float* inv_lenpow, int64_t n_lenpow, uint32_t* live_acc, int32_t* live,
                         EosArgs* ea) {
  FK_CHECK_ARG(eos < (1LL << 31), "%s: need eos < 2^31 (eos=%lld)", fn, (long long)eos);
  *ea = EosArgs{eos < 0 ? -1 : (int)eos, fin, len, inv_lenpow, (int)n_lenpow, live_acc, live};
  return FK_OK;
}

template <bool EOS, bool NUCLEUS>
static int sample_topk(const char* fn, bool ptrs, const float* logits, int64_t ld, int64_t B, int64_t V, float temperature, int64_t top_k, float top_p,
                       const uint64_t* seed, int64_t* step, int32_t* pos_inc, int64_t* cur, int64_t* out, int64_t out_ld, int64_t out_cols, uint32_t* ticket,
                       const EosArgs& ea, void* stream) {
  FK_CHECK_ARG(out == nullptr || (out_cols > 0 && out_cols <= out_ld), "%s: out given without its width (out_cols=%lld, out_ld=%lld)", fn, (long long)out_cols,
               (long long)out_ld);
  FK_CHECK_ARG(ptrs, "%s: null pointer", fn);
  if (const int rc = check_logit_rows(fn, B, V, ld); rc != FK_OK) return rc;
  FK_CHECK_ARG(temperature > 0.0f, "%s: need temperature > 0 (temperature=%g)", fn, (double)temperature);      // refuses NaN as well
  FK_CHECK_ARG(!NUCLEUS || (top_p > 0.0f && top_p <= 1.0f), "%s: need 0 < top_p <= 1 (top_p=%g)", fn, (double)top_p);      // refuses NaN as well
  hipLaunchKernelGGL((sample_topk_kernel<EOS, NUCLEUS>), dim3((unsigned)B), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, logits, ld, (int)V, 1.0f / temperature,
                     (int)(top_k > 0 && top_k < V ? top_k : 0), top_p, (const unsigned long long*)seed, step, pos_inc, cur, out, out_ld, out_cols, ticket, ea);
  FK_CHECK_LAUNCH(fn);
  return FK_OK;
}

static int check_attn_decode_beam(const char* fn, bool ptrs, const void* kv, int64_t kv_bs, int64_t kv_rs, int64_t anc_ld, int64_t W, int64_t H, int64_t D, int dtype) {
  FK_CHECK_ARG((dtype == FK_F32 || dtype == FK_BF16) && ptrs && W > 0 && W < 65536 && H > 0 && H < 65536 && anc_ld > 0, "%s: bad arguments", fn);
  FK_CHECK_ARG(D == 16 || D == 32 || D == 64 || D == 128, "%s: head_dim %lld not in {16, 32, 64, 128}", fn, (long long)D);
  const int64_t vn = dtype == FK_BF16 ? 8 : 4;
  FK_CHECK_ARG(((uintptr_t)kv & 15) == 0 && kv_bs % vn == 0 && kv_rs % vn == 0 && kv_rs >= 2 * H * D,
               "%s: cache rows must be 16-byte aligned and hold key|value (kv_bs=%lld, kv_rs=%lld)", fn, (long long)kv_bs, (long long)kv_rs);
  return FK_OK;
}

// grid = (H, rows): GROUPED rows = S * W, the beams of S sentences; otherwise the W beams of one sentence, and tmax and append are not read
template <bool GROUPED>
static int launch_attn_decode_beam(const char* fn, const void* q, int64_t q_bs, void* kv, int64_t kv_bs, int64_t kv_rs, int64_t tmax, const int32_t* anc, int64_t anc_ld,
                                   void* out, int64_t o_bs, const int32_t* pos, int64_t rows, int64_t W, int64_t H, int64_t D, float scale, int append, int dtype,
                                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)H, (unsigned)rows), block(256);
  FK_BY_DTYPE(dtype, T, FK_BY_HEAD_DIM(D, DD, hipLaunchKernelGGL((attn_decode_beam_kernel<T, DD, GROUPED>), grid, block, 0, s, (const T*)q, q_bs, (T*)kv, kv_bs, kv_rs,
                                                          (int)tmax, anc, anc_ld, (T*)out, o_bs, pos, (int)W, (int)H, scale, append)));
  FK_CHECK_LAUNCH(fn);
  return FK_OK;
}

// GROUPED: one block per sentence, S sentences whose rows lie group_stride apart, and a ticket; otherwise S = 1, group_stride = 0 and no ticket
template <bool GROUPED, bool EOS>
static int beam_select(const char* fn, bool ptrs, const float* top_lp, const int64_t* top_id, int64_t row_stride, int64_t group_stride, int64_t S, int64_t W, int64_t k,
                       float* scores, const uint64_t* seed, int64_t* step, const int32_t* pos, int32_t* pos_inc, int64_t* cur, int32_t* parent_log, int64_t* tok_log,
                       int64_t log_rows, int32_t* anc, int64_t anc_ld, uint32_t* ticket, const EosArgs& ea, void* stream) {
  FK_CHECK_ARG(ptrs, "%s: null pointer", fn);
  FK_CHECK_ARG(W >= 1 && W <= BEAM_MAX_W && k >= W && k <= BEAM_MAX_K, "%s: need 1 <= W <= %d and W <= k <= %d (W=%lld k=%lld)", fn, BEAM_MAX_W, BEAM_MAX_K,
               (long long)W, (long long)k);
  FK_CHECK_ARG(S >= 1 && S * W < 65536, "%s: need S >= 1 and S * W < 65536 rows (S=%lld W=%lld)", fn, (long long)S, (long long)W);
  FK_CHECK_ARG((row_stride == 0 || row_stride >= k) && (!GROUPED || group_stride >= (W - 1) * row_stride + k),
               "%s: rows overlap (row_stride=%lld group_stride=%lld k=%lld)", fn, (long long)row_stride, (long long)group_stride, (long long)k);
  FK_CHECK_ARG(anc_ld > 0 && log_rows >= 0 && (log_rows == 0 || (parent_log && tok_log)), "%s: bad arguments (anc_ld=%lld log_rows=%lld)", fn, (long long)anc_ld,
               (long long)log_rows);
  hipLaunchKernelGGL((beam_select_kernel<GROUPED, EOS>), dim3((unsigned)S), dim3(BEAM_SELECT_THREADS), 0, (hipStream_t)stream, top_lp, top_id, row_stride, group_stride,
                     (int)W, (int)k, scores, (const unsigned long long*)seed, step, pos, pos_inc, cur, parent_log, tok_log, log_rows, anc, anc_ld, ticket, ea);
  FK_CHECK_LAUNCH(fn);
  return FK_OK;
}

extern "C" {

int fk_gpt_embed_step(const int64_t* idx, const float* wte, const float* wpe, const int32_t* pos, void* out, int64_t B, int64_t dim,
                      int64_t vocab, int dtype, void* stream) {
  FK_CHECK_ARG((dtype == FK_F32 || dtype == FK_BF16) && idx && wte && wpe && pos && out && B > 0 && dim > 0 && vocab > 0, "fk_gpt_embed_step: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  FK_BY_DTYPE(dtype, T, hipLaunchKernelGGL(gpt_embed_step_kernel<T>, dim3((unsigned)B), dim3(128), 0, s, idx, wte, wpe, pos, (T*)out, (int)dim, vocab));
  FK_CHECK_LAUNCH("fk_gpt_embed_step");
  return FK_OK;
}

int fk_kv_append(const void* qkv, void* kv, const int32_t* pos, int64_t B, int64_t d, int64_t tmax, int dtype, void* stream) {
  FK_CHECK_ARG((dtype == FK_F32 || dtype == FK_BF16) && qkv && kv && pos && B > 0 && d > 0 && tmax > 0, "fk_kv_append: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  FK_BY_DTYPE(dtype, T, hipLaunchKernelGGL(kv_append_kernel<T>, dim3((unsigned)B), dim3(256), 0, s, (const T*)qkv, (T*)kv, pos, (int)d, tmax));
  FK_CHECK_LAUNCH("fk_kv_append");
  return FK_OK;
}

int fk_attn_decode(const void* q, int64_t q_bs, const void* kv, int64_t kv_bs, int64_t kv_rs, void* out, int64_t o_bs, const int32_t* pos,
                   int64_t B, int64_t H, int64_t D, float scale, int dtype, void* stream) {
  FK_CHECK_ARG((dtype == FK_F32 || dtype == FK_BF16) && q && kv && out && pos && B > 0 && H > 0, "fk_attn_decode: bad arguments");
  FK_CHECK_ARG(D == 16 || D == 32 || D == 64 || D == 128, "fk_attn_decode: head_dim %lld not in {16, 32, 64, 128}", (long long)D);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)H, (unsigned)B), block(256);
  FK_BY_DTYPE(dtype, T, FK_BY_HEAD_DIM(D, DD, hipLaunchKernelGGL((attn_decode_kernel<T, DD>), grid, block, 0, s, (const T*)q, q_bs, (const T*)kv, kv_bs, kv_rs, (T*)out,
                                                          o_bs, pos, (int)H, scale)));
  FK_CHECK_LAUNCH("fk_attn_decode");
  return FK_OK;
}

int fk_sample_topk(const float* logits, int64_t ld, int64_t B, int64_t V, float temperature, int64_t top_k, const uint64_t* seed, int64_t* step,
                   int32_t* pos_inc, int64_t* cur, int64_t* out, int64_t out_ld, int64_t out_cols, uint32_t* ticket, void* stream) {
  return sample_topk<false, false>("fk_sample_topk", logits && seed && step && cur && ticket, logits, ld, B, V, temperature, top_k, 1.0f, seed, step, pos_inc, cur, out,
                                   out_ld, out_cols, ticket, EosArgs{}, stream);
}

int fk_attn_decode_beam(const void* q, int64_t q_bs, const void* kv, int64_t kv_bs, int64_t kv_rs, const int32_t* anc, int64_t anc_ld, void* out,
                        int64_t o_bs, const int32_t* pos, int64_t W, int64_t H, int64_t D, float scale, int dtype, void* stream) {
  const int rc = check_attn_decode_beam("fk_attn_decode_beam", q && kv && anc && out && pos, kv, kv_bs, kv_rs, anc_ld, W, H, D, dtype);
  if (rc != FK_OK) return rc;
  return launch_attn_decode_beam<false>("fk_attn_decode_beam", q, q_bs, (void*)kv, kv_bs, kv_rs, 0, anc, anc_ld, out, o_bs, pos, W, W, H, D, scale, 0, dtype, stream);
}

int fk_beam_topk(const float* logits, int64_t ld, int64_t R, int64_t V, float temperature, int64_t k, float* top_lp, int64_t* top_id, void* stream) {
  FK_CHECK_ARG(logits && top_lp && top_id, "fk_beam_topk: null pointer");
  if (const int rc = check_logit_rows("fk_beam_topk", R, V, ld); rc != FK_OK) return rc;
  FK_CHECK_ARG(temperature > 0.0f, "fk_beam_topk: need temperature > 0 (temperature=%g)", (double)temperature);      // refuses NaN as well
  FK_CHECK_ARG(k >= 1 && k <= BEAM_MAX_K && k <= V, "fk_beam_topk: k=%lld outside 1 .. min(%d, V=%lld)", (long long)k, BEAM_MAX_K, (long long)V);
  hipLaunchKernelGGL(beam_topk_kernel, dim3((unsigned)R), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, logits, ld, (int)V, 1.0f / temperature, (int)k,
                     top_lp, top_id);
  FK_CHECK_LAUNCH("fk_beam_topk");
  return FK_OK;
}

int fk_beam_select(const float* top_lp, const int64_t* top_id, int64_t row_stride, int64_t W, int64_t k, float* scores, const uint64_t* seed,
                   int64_t* step, const int32_t* pos, int32_t* pos_inc, int64_t* cur, int32_t* parent_log, int64_t* tok_log, int64_t log_rows,
                   int32_t* anc, int64_t anc_ld, void* stream) {
  return beam_select<false, false>("fk_beam_select", top_lp && top_id && scores && seed && step && pos && cur && anc, top_lp, top_id, row_stride, 0, 1, W, k, scores,
                                   seed, step, pos, pos_inc, cur, parent_log, tok_log, log_rows, anc, anc_ld, nullptr, EosArgs{}, stream);
}

int fk_attn_decode_beam_grouped(const void* qkv, int64_t q_bs, void* kv, int64_t kv_bs, int64_t kv_rs, int64_t tmax, const int32_t* anc, int64_t anc_ld,
                                void* out, int64_t o_bs, const int32_t* pos, int64_t S, int64_t W, int64_t H, int64_t D, float scale, int append, int dtype,
                                void* stream) {
  const int rc = check_attn_decode_beam("fk_attn_decode_beam_grouped", qkv && kv && anc && out && pos, kv, kv_bs, kv_rs, anc_ld, W, H, D, dtype);
  if (rc != FK_OK) return rc;
  FK_CHECK_ARG(S >= 1 && S < 65536 && S * W < 65536, "fk_attn_decode_beam_grouped: need S >= 1 and S * W < 65536 rows (S=%lld W=%lld)", (long long)S, (long long)W);
  FK_CHECK_ARG(tmax > 0 && tmax < (1LL << 31), "fk_attn_decode_beam_grouped: tmax=%lld", (long long)tmax);
  FK_CHECK_ARG(!append || (((uintptr_t)qkv & 15) == 0 && q_bs % (dtype == FK_BF16 ? 8 : 4) == 0 && q_bs >= 3 * H * D),
               "fk_attn_decode_beam_grouped: append reads [q | k | v] rows as 16-byte vectors (q_bs=%lld)", (long long)q_bs);
  return launch_attn_decode_beam<true>("fk_attn_decode_beam_grouped", qkv, q_bs, kv, kv_bs, kv_rs, tmax, anc, anc_ld, out, o_bs, pos, S * W, W, H, D, scale, append, dtype,
                                       stream);
}

int fk_beam_select_grouped(const float* top_lp, const int64_t* top_id, int64_t row_stride, int64_t group_stride, int64_t S, int64_t W, int64_t k,
                           float* scores, const uint64_t* seed, int64_t* step, const int32_t* pos, int32_t* pos_inc, int64_t* cur, int32_t* parent_log,
                           int64_t* tok_log, int64_t log_rows, int32_t* anc, int64_t anc_ld, uint32_t* ticket, void* stream) {
  return beam_select<true, false>("fk_beam_select_grouped", top_lp && top_id && scores && seed && step && pos && cur && anc && ticket, top_lp, top_id, row_stride,
                                  group_stride, S, W, k, scores, seed, step, pos, pos_inc, cur, parent_log, tok_log, log_rows, anc, anc_ld, ticket, EosArgs{}, stream);
}

int fk_beam_select_eos(const float* top_lp, const int64_t* top_id, int64_t row_stride, int64_t group_stride, int64_t S, int64_t W, int64_t k,
                       float* scores, const uint64_t* seed, int64_t* step, const int32_t* pos, int32_t* pos_inc, int64_t* cur, int32_t* parent_log,
                       int64_t* tok_log, int64_t log_rows, int32_t* anc, int64_t anc_ld, uint32_t* ticket, int64_t eos, int32_t* fin, int32_t* len,
                       const float* inv_lenpow, int64_t n_lenpow, uint32_t* live_acc, int32_t* live, void* stream) {
  FK_CHECK_ARG(n_lenpow >= 1 && n_lenpow < (1LL << 31), "fk_beam_select_eos: need 1 <= n_lenpow < 2^31 (n_lenpow=%lld)", (long long)n_lenpow);
  EosArgs ea;
  if (const int rc = make_eos_args("fk_beam_select_eos", eos, fin, len, inv_lenpow, n_lenpow, live_acc, live, &ea); rc != FK_OK) return rc;
  return beam_select<true, true>("fk_beam_select_eos", top_lp && top_id && scores && seed && step && pos && cur && anc && ticket && fin && len && inv_lenpow && live_acc && live,
                                 top_lp, top_id, row_stride, group_stride, S, W, k, scores, seed, step, pos, pos_inc, cur, parent_log, tok_log, log_rows, anc, anc_ld,
                                 ticket, ea, stream);
}

int fk_beam_backtrack(const int32_t* parent_log, const int64_t* tok_log, int64_t log_rows, int64_t S, int64_t W, const int64_t* step, const float* scores,
                      const int32_t* len, const float* inv_lenpow, int64_t n_lenpow, int64_t* out_ids, int64_t out_ld, int64_t out_cols, int64_t t0,
                      int64_t pad, float* out_scores, int32_t* out_len, void* stream) {
  FK_CHECK_ARG(parent_log && tok_log && step && scores && len && inv_lenpow && out_ids && out_scores && out_len, "fk_beam_backtrack: null pointer");
  FK_CHECK_ARG(W >= 1 && W <= BEAM_MAX_W && S >= 1 && S * W < 65536, "fk_beam_backtrack: need 1 <= W <= %d, S >= 1 and S * W < 65536 rows (S=%lld W=%lld)",
               BEAM_MAX_W, (long long)S, (long long)W);
  FK_CHECK_ARG(n_lenpow >= 1 && n_lenpow < (1LL << 31) && log_rows >= 1, "fk_beam_backtrack: need n_lenpow >= 1 and log_rows >= 1 (n_lenpow=%lld log_rows=%lld)",
               (long long)n_lenpow, (long long)log_rows);
  FK_CHECK_ARG(t0 >= 0 && out_cols >= t0 && out_cols > 0 && out_ld >= out_cols,
               "fk_beam_backtrack: rows of out_cols=%lld ids (stride out_ld=%lld) must hold the prompt t0=%lld and must not overlap", (long long)out_cols,
               (long long)out_ld, (long long)t0);
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3((unsigned)S), dim3(BACKTRACK_THREADS), 0, (hipStream_t)stream, parent_log, tok_log, log_rows, (int)W, step,
                     scores, len, inv_lenpow, (int)n_lenpow, out_ids, out_ld, out_cols, t0, pad, out_scores, out_len);
  FK_CHECK_LAUNCH("fk_beam_backtrack");
  return FK_OK;
}

int fk_sample_topk_eos(const float* logits, int64_t ld, int64_t B, int64_t V, float temperature, int64_t top_k, const uint64_t* seed, int64_t* step,
                       int32_t* pos_inc, int64_t* cur, int64_t* out, int64_t out_ld, int64_t out_cols, uint32_t* ticket, int64_t eos, int32_t* done,
                       int32_t* len, uint32_t* live_acc, int32_t* live, void* stream) {
  EosArgs ea;
  if (const int rc = make_eos_args("fk_sample_topk_eos", eos, done, len, nullptr, 0, live_acc, live, &ea); rc != FK_OK) return rc;
  return sample_topk<true, false>("fk_sample_topk_eos", logits && seed && step && cur && ticket && done && len && live_acc && live, logits, ld, B, V, temperature, top_k,
                                  1.0f, seed, step, pos_inc, cur, out, out_ld, out_cols, ticket, ea, stream);
}

int fk_sample_topp(const float* logits, int64_t ld, int64_t B, int64_t V, float temperature, int64_t top_k, float top_p, const uint64_t* seed, int64_t* step,
                   int32_t* pos_inc, int64_t* cur, int64_t* out, int64_t out_ld, int64_t out_cols, uint32_t* ticket, int64_t eos, int32_t* done, int32_t* len,
                   uint32_t* live_acc, int32_t* live, void* stream) {
  const bool ptrs = logits && seed && step && cur && ticket;
  if (!done) {                                           // the plain mode: no end-of-text state at all, eos is not read
    FK_CHECK_ARG(!len && !live_acc && !live, "fk_sample_topp: len / live_acc / live given without done (all four or none)");
    return sample_topk<false, true>("fk_sample_topp", ptrs, logits, ld, B, V, temperature, top_k, top_p, seed, step, pos_inc, cur, out, out_ld, out_cols, ticket,
                                    EosArgs{}, stream);
  }
  FK_CHECK_ARG(len && live_acc && live, "fk_sample_topp: done given without len / live_acc / live (all four or none)");
  EosArgs ea;
  if (const int rc = make_eos_args("fk_sample_topp", eos, done, len, nullptr, 0, live_acc, live, &ea); rc != FK_OK) return rc;
  return sample_topk<true, true>("fk_sample_topp", ptrs, logits, ld, B, V, temperature, top_k, top_p, seed, step, pos_inc, cur, out, out_ld, out_cols, ticket, ea, stream);
}

int fk_logit_rules(float* logits, int64_t ld, int64_t R, int64_t V, float penalty, int64_t ngram, int64_t min_new, int64_t eos, const int64_t* step,
                   const int64_t* cur, int32_t* hist, int32_t* hist2, int64_t hist_ld, int64_t t0, int64_t steps, const int32_t* parent_log,
                   int64_t log_rows, int64_t W, int broadcast, void* stream) {
  FK_CHECK_ARG(logits && step && cur && hist, "fk_logit_rules: null pointer");
  FK_CHECK_ARG((hist2 == nullptr) == (parent_log == nullptr), "fk_logit_rules: hist2 and parent_log select the beam mode together (both or none)");
  if (const int rc = check_logit_rows("fk_logit_rules", R, V, ld); rc != FK_OK) return rc;
  FK_CHECK_ARG(penalty > 0.0f && penalty <= 3.402823466e38f, "fk_logit_rules: need a finite penalty > 0 (penalty=%g)", (double)penalty);      // refuses NaN as well
  FK_CHECK_ARG(ngram >= 0 && ngram < (1LL << 31) && min_new >= 0 && min_new < (1LL << 31) && eos < (1LL << 31),
               "fk_logit_rules: need 0 <= ngram, min_new < 2^31 and eos < 2^31 (ngram=%lld min_new=%lld eos=%lld)", (long long)ngram, (long long)min_new, (long long)eos);
  FK_CHECK_ARG(t0 >= 0 && steps >= 0 && t0 + steps <= RULES_MAX_HIST && hist_ld >= t0 + steps,
               "fk_logit_rules: a history row holds t0 + steps <= %d ids and hist_ld >= that (t0=%lld steps=%lld hist_ld=%lld)", RULES_MAX_HIST, (long long)t0,
               (long long)steps, (long long)hist_ld);
  if (hist2) {
    FK_CHECK_ARG(W >= 1 && W <= BEAM_MAX_W && log_rows >= 0, "fk_logit_rules: need 1 <= W <= %d and log_rows >= 0 (W=%lld log_rows=%lld)", BEAM_MAX_W, (long long)W,
                 (long long)log_rows);
    FK_CHECK_ARG(broadcast ? R * W < 65536 : R % W == 0, "fk_logit_rules: the rows are S sentences x W beams, or S with broadcast (R=%lld W=%lld)", (long long)R, (long long)W);
  } else {
    FK_CHECK_ARG(!broadcast, "fk_logit_rules: broadcast belongs to the beam mode");
  }
  const float inv_p = (float)(1.0 / (double)penalty);
  hipLaunchKernelGGL(logit_rules_kernel, dim3((unsigned)R), dim3(RULES_THREADS), 0, (hipStream_t)stream, logits, ld, (int)V, penalty, inv_p, (int)ngram, (int)min_new,
                     eos < 0 ? -1 : (int)eos, step, cur, hist, hist2, hist_ld, (int)t0, parent_log, log_rows, (int)W, broadcast);
  FK_CHECK_LAUNCH("fk_logit_rules");
  return FK_OK;
}

}  // extern "C"
