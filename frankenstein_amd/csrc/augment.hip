// augment.hip — training-time signal augmentation drawn inside the patch tokeniser: white noise, a per-trial channel offset, masked
// time spans, dropped electrodes and a small shift in time, in the one pass through LDS that fk_patchify makes anyway.  The rule
// (build-defined: the reference has no augmentation; restated in float64 in tests/augment_ref.py) is the comment of
// fk_augment_patchify in include/franken_hip.h.  Every draw is a pure function of (seed, step, sample, frame, channel): Philox4x32-10,
// key = the two device words [seed, step], counter = (i0, i1, b, 0xA0610000 | kind).  No mask and no noise tensor exists.
//
// augment_patchify_kernel has patchify_kernel's frame: a workgroup per (sample, patch), a [P][C + 1] fp32 slab, a transposed store.
//   1. (MASK, time_shift > 0) the sample's shift, drawn by every wave for itself (uniform: see the kernel).
//   2. the staging loop reads the SHIFTED source rows (zeros outside [0, T)), AUG_BATCH loads in flight per thread; then the sample's
//      spans (one lane each) and the 2 * ceil(C / 4) Philox blocks of its offset normals and electrode keep bits go into LDS, once per
//      workgroup, amortised over the P rows.
//   3. (MASK or PAD) one wave per row: out of range, inside a span (lane m holds span m: one vote), or (PAD) all-zero by a wave vote
//      over the staged row -> dead row.
//   4. (NOISE) one Philox block per four consecutive channels of a live row, computed by the thread that owns those four slab
//      elements: src + white_sd * n_w + offset_sd * n_o.  With C % 4 != 0 the last block of a row uses its first C & 3 normals.
//   5. the store of patchify_kernel; the masks come last, here: an element of a dead row or of a dropped channel leaves as +0.
// NOISE / MASK / PAD are template flags picked on the host from the knobs, so a knob that is off costs nothing: without NOISE no
// white-noise block is ever computed, with all three off the kernel is patchify_kernel.  PAD is only set together with NOISE: without
// noise a padding frame goes through as the zeros it is.  Plain stores, no atomics, nothing read on the host: same bits on every run.
// The Philox loops carry `vectorize(disable)`: at -O3 the loop vectorizer otherwise runs two blocks per thread in packed fp32
// (v_pk_mul_f32 / v_pk_add_f32 with op_sel), the instruction forms this library keeps out of its code objects.
#include <math.h>

#include "fk_common.h"

namespace {

constexpr int AUG_MAX_SPANS = 8;
constexpr int AUG_BATCH = 8;               // staging loads in flight per thread
constexpr unsigned AUG_TAG = 0xA0610000u;
constexpr int AUG_WHITE = 1, AUG_OFFSET = 2, AUG_CHAN = 3, AUG_SPAN = 4, AUG_SHIFT = 5;
constexpr size_t AUG_LDS_MAX = 159 * 1024;   // slab (at most 64 KiB) + the per-channel and per-row tables; gfx950 has 160 KiB

struct AugArgs {
  const float* x;
  void* tok;
  const unsigned* words;
  int T, C, P, ldp, C4;
  float white_sd, offset_sd;
  unsigned thresh;
  int S, n_masks, Lmax;
};

// two standard normals from two words (Box-Muller).  u1 has 24 significant bits ((wa >> 9) + 0.5 over 2^23): exact in fp32, never 0 or 1
FK_DEV void aug_normals(unsigned wa, unsigned wb, float& n0, float& n1) {
  const float u1 = ((float)(wa >> 9) + 0.5f) * 0x1p-23f;
  const float u2 = (float)(wb >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);
  n0 = r * cs;
  n1 = r * sn;
}

FK_DEV void aug_block(unsigned k0, unsigned k1, unsigned i0, unsigned i1, unsigned b, int kind, unsigned (&c)[4]) {
  c[0] = i0; c[1] = i1; c[2] = b; c[3] = AUG_TAG | (unsigned)kind;
  philox4x32_10(k0, k1, c);
}

template <typename E, bool NOISE, bool MASK, bool PAD>
__global__ __launch_bounds__(FK_TPB) void augment_patchify_kernel(AugArgs a) {
  extern __shared__ float slab[];                    // [P][C + 1], then off [4 C4], dead [P], keep [4 C4] bytes
  __shared__ int sc[2 * AUG_MAX_SPANS];              // (start, len) per span of the sample
  const int T_ = a.T, C = a.C, P = a.P, ldp = a.ldp, ld = C + 1, C4 = a.C4;
  float* off = slab + P * ld;
  int* dead = (int*)(off + 4 * C4);
  unsigned char* keep = (unsigned char*)(dead + P);
  const int nT = T_ / P;
  const int b = blockIdx.x / nT, t0 = (blockIdx.x % nT) * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned k0 = 0, k1 = 0;
  if constexpr (NOISE || MASK) { k0 = a.words[0]; k1 = a.words[1]; }
  int shift = 0;
  if constexpr (MASK) {
    // The staging loop needs the shift before its first load.  Every wave draws it for itself: the block is uniform over the sample, so
    // this is the instruction stream of one lane doing it, without the barrier and the LDS round trip in front of the loads; with
    // time_shift == 0 nothing stands in front of them at all.
    if (a.S > 0) {
      unsigned w[4];
      aug_block(k0, k1, 0, 0, b, AUG_SHIFT, w);
      shift = (int)(((uint64_t)(w[0] >> 8) * (uint64_t)(2 * (int64_t)a.S + 1)) >> 24) - a.S;
    }
  }
  const float* xb = a.x + (int64_t)b * T_ * C;
  // element i of the patch: the value of the shifted source row (an unconditional load of the row clamped into [0, T), then a select:
  // a conditional load keeps the loads of a batch from being issued together) and its place in the slab
  auto fetch = [&](int i, float& v, int& at) {
    const int r = i / C, c = i - r * C;
    const int64_t ts = (int64_t)t0 + r - shift;
    const int64_t tc = !MASK ? ts : (ts < 0 ? 0 : (ts >= T_ ? T_ - 1 : ts));
    v = xb[tc * C + c];
    if (MASK && tc != ts) v = 0.0f;
    at = r * ld + c;
  };
  int i0 = tid;
  for (; i0 + (AUG_BATCH - 1) * FK_TPB < P * C; i0 += AUG_BATCH * FK_TPB) {      // AUG_BATCH loads in flight per thread
    float v[AUG_BATCH];
    int at[AUG_BATCH];
#pragma unroll
    for (int k = 0; k < AUG_BATCH; ++k) fetch(i0 + k * FK_TPB, v[k], at[k]);
#pragma unroll
    for (int k = 0; k < AUG_BATCH; ++k) slab[at[k]] = v[k];
  }
  for (; i0 < P * C; i0 += FK_TPB) {
    float v;
    int at;
    fetch(i0, v, at);
    slab[at] = v;
  }
  if constexpr (NOISE) {
    if (a.offset_sd > 0.0f) {
#pragma clang loop vectorize(disable)
      for (int j = tid; j < C4; j += FK_TPB) {
        unsigned w[4];
        float n[4];
        aug_block(k0, k1, j, 0, b, AUG_OFFSET, w);
        aug_normals(w[0], w[1], n[0], n[1]);
        aug_normals(w[2], w[3], n[2], n[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) off[4 * j + k] = a.offset_sd * n[k];
      }
    }
  }
  if constexpr (MASK) {
    if (tid < a.n_masks) {                               // span tid of the sample: (start, len) through LDS
      unsigned w[4];
      aug_block(k0, k1, tid, 0, b, AUG_SPAN, w);
      const int len = (int)(((uint64_t)(w[0] >> 8) * (uint64_t)(a.Lmax + 1)) >> 24);
      sc[2 * tid] = (int)(((uint64_t)(w[1] >> 8) * (uint64_t)((int64_t)T_ - len + 1)) >> 24);
      sc[2 * tid + 1] = len;
    }
    if (a.thresh > 0u) {
#pragma clang loop vectorize(disable)
      for (int j = tid; j < C4; j += FK_TPB) {
        unsigned w[4];
        aug_block(k0, k1, j, 0, b, AUG_CHAN, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) keep[4 * j + k] = w[k] >= a.thresh;
      }
    }
  }
  __syncthreads();
  if constexpr (MASK || PAD) {
    int64_t st = 0, en = 0;                              // lane m holds span m: a row is tested against all spans by one vote
    if constexpr (MASK) {
      if (lane < a.n_masks) { st = sc[2 * lane]; en = st + sc[2 * lane + 1]; }
    }
    for (int r = wave; r < P; r += FK_TPB / 64) {       // r is uniform over the wave
      bool d = false;
      if constexpr (MASK) {
        const int64_t t = (int64_t)t0 + r, ts = t - shift;
        d = ts < 0 || ts >= T_ || __any(t >= st && t < en);
      }
      if constexpr (PAD) {
        bool nz = false;
        for (int c = lane; c < C; c += 64) nz = nz | (slab[r * ld + c] != 0.0f);
        d = d || !__any(nz);
      }
      if (lane == 0) dead[r] = d;
    }
    __syncthreads();
  }
  if constexpr (NOISE) {
#pragma clang loop vectorize(disable)
    for (int j = tid; j < P * C4; j += FK_TPB) {
      const int r = j / C4, q = j - r * C4, c0 = 4 * q;
      if constexpr (PAD || MASK) {
        if (dead[r]) continue;                           // the store writes the +0: no Philox block for a dead row
      }
      float* p = slab + r * ld + c0;
      float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (a.white_sd > 0.0f) {
        unsigned w[4];
        aug_block(k0, k1, (unsigned)(t0 + r), q, b, AUG_WHITE, w);
        aug_normals(w[0], w[1], n[0], n[1]);
        aug_normals(w[2], w[3], n[2], n[3]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (c0 + k < C) {
          float v = p[k];
          if (a.white_sd > 0.0f) v = __builtin_fmaf(a.white_sd, n[k], v);      // a term whose sd is 0 is skipped: x passes bit for bit
          if (a.offset_sd > 0.0f) v += off[c0 + k];
          p[k] = v;
        }
      }
    }
    __syncthreads();
  }
  // the masks come last, in the store: a dead row or a dropped channel leaves as +0 whatever the slab holds
  const bool drop = MASK && a.thresh > 0u;
  E* dst = (E*)a.tok + ((int64_t)blockIdx.x * C) * ldp;
  for (int i = tid; i < C * ldp; i += FK_TPB) {
    const int c = i / ldp, p = i - c * ldp;
    const int pc = p < P ? p : P - 1;                     // unconditional LDS reads, then selects
    float v = slab[pc * ld + c];
    bool z = p >= P;
    if constexpr (MASK || PAD) z = z || dead[pc] != 0;
    if constexpr (MASK) z = z || (drop && keep[c] == 0);
    v = z ? 0.0f : v;
    dst[i] = from_f32<E>(v);
  }
}

template <auto Kernel>
void aug_go(const AugArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  static const bool once = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)AUG_LDS_MAX) == hipSuccess;
  (void)once;
  hipLaunchKernelGGL(Kernel, grid, dim3(FK_TPB), lds, s, a);
}

template <typename E>
void aug_launch(const AugArgs& a, bool noise, bool mask, bool pad, dim3 grid, size_t lds, hipStream_t s) {
  if (noise && mask && pad) return aug_go<augment_patchify_kernel<E, true, true, true>>(a, grid, lds, s);
  if (noise && mask) return aug_go<augment_patchify_kernel<E, true, true, false>>(a, grid, lds, s);
  if (noise && pad) return aug_go<augment_patchify_kernel<E, true, false, true>>(a, grid, lds, s);
  if (noise) return aug_go<augment_patchify_kernel<E, true, false, false>>(a, grid, lds, s);
  if (mask) return aug_go<augment_patchify_kernel<E, false, true, false>>(a, grid, lds, s);
  aug_go<augment_patchify_kernel<E, false, false, false>>(a, grid, lds, s);
}

}  // namespace

extern "C" {

int fk_augment_patchify(const float* x, void* tok, int64_t B, int64_t T, int64_t C, int64_t P, int64_t ldp, const fk_augment_cfg* cfg,
                        const uint32_t* words, int dtype, void* stream) {
  FK_DT_CHECK("fk_augment_patchify");
  FK_CHECK_ARG(x && tok && cfg && words, "fk_augment_patchify: null pointer");
  FK_CHECK_ARG(B > 0 && T > 0 && C > 0 && P > 0 && T % P == 0 && ldp >= P, "fk_augment_patchify: bad shape (T %% P must be 0, ldp >= P)");
  const size_t sh = (size_t)P * (C + 1) * sizeof(float);
  FK_CHECK_ARG(sh <= 65536, "fk_augment_patchify: P*(C+1) slab of %zu bytes exceeds 64 KiB LDS", sh);
  const int64_t lim = 1LL << 31;
  FK_CHECK_ARG(T < lim && ldp < lim / C && B * (T / P) < lim, "fk_augment_patchify: sizes exceed int32");
  FK_CHECK_ARG(cfg->white_sd >= 0.0f && isfinite(cfg->white_sd) && cfg->offset_sd >= 0.0f && isfinite(cfg->offset_sd),
               "fk_augment_patchify: white_sd %g / offset_sd %g must be finite and >= 0", (double)cfg->white_sd, (double)cfg->offset_sd);
  FK_CHECK_ARG(cfg->chan_drop_p >= 0.0f && cfg->chan_drop_p < 1.0f, "fk_augment_patchify: chan_drop_p %g outside [0, 1)", (double)cfg->chan_drop_p);
  FK_CHECK_ARG(cfg->n_time_masks >= 0 && cfg->n_time_masks <= AUG_MAX_SPANS, "fk_augment_patchify: n_time_masks %d outside [0, %d]", cfg->n_time_masks,
               AUG_MAX_SPANS);
  FK_CHECK_ARG(cfg->time_mask_len >= 0 && cfg->time_mask_len <= T, "fk_augment_patchify: time_mask_len %d outside [0, T]", cfg->time_mask_len);
  FK_CHECK_ARG(cfg->time_shift >= 0 && cfg->time_shift < T, "fk_augment_patchify: time_shift %d outside [0, T)", cfg->time_shift);
  FK_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)words & 3) == 0 && ((uintptr_t)tok & (dtype == FK_BF16 ? 1 : 3)) == 0,
               "fk_augment_patchify: misaligned pointer");
  double th = floor((double)cfg->chan_drop_p * 4294967296.0);
  if (th > 4294967295.0) th = 4294967295.0;
  const int C4 = (int)fk_cdiv(C, 4);
  AugArgs a{x, tok, words, (int)T, (int)C, (int)P, (int)ldp, C4, cfg->white_sd, cfg->offset_sd, (unsigned)th, cfg->time_shift,
            cfg->time_mask_len > 0 ? cfg->n_time_masks : 0, cfg->time_mask_len};
  const bool noise = a.white_sd > 0.0f || a.offset_sd > 0.0f;
  const bool mask = a.thresh > 0u || a.S > 0 || a.n_masks > 0;
  const bool pad = noise && cfg->keep_padding != 0;
  const size_t lds = sh + (size_t)C4 * 4 * sizeof(float) + (size_t)P * sizeof(int) + (size_t)C4 * 4;
  FK_CHECK_ARG(lds <= AUG_LDS_MAX, "fk_augment_patchify: slab and tables of %zu bytes exceed the LDS", lds);
  const dim3 grid((unsigned)(B * (T / P)));
  FK_BY_DTYPE(dtype, E, aug_launch<E>(a, noise, mask, pad, grid, lds, (hipStream_t)stream));
  FK_CHECK_LAUNCH("fk_augment_patchify");
  return FK_OK;
}

}  // extern "C"
