// mlp_fused.hip — the SwiGLU MLP's data-gradient chain as ONE attention-shaped kernel (gfx950 only).
//
//   reference call sites: models/brainformer.py:119-124 (MLP.forward: w2(silu(w1 x) * w3 x)), autograd of it.
//   replaces, in the backward of the fused SwiGLU path (engine.MlpBranch.backward):
//       dh13 = fk_gemm_nt_dswiglu(dy, W2T, h13)        (dg = dy W2T^T never stored; dh13 written: 1.2 GB per cfg2 layer)
//       dx   = fk_gemm_nt(dh13, W13T)                  (dh13 read back: 1.2 GB)
//   by one launch that keeps dh13 in registers between the two products (it is still written once: the weight gradients need it).
//
// The token is on the LANE, as the query is in the attention kernels: with C^T = A B (A: weight rows from LDS, B: activations from
// registers) an accumulator tile holds 32 output features x 32 tokens, lane = token.  Per workgroup of 4 waves = 128 tokens
// (one wave per SIMD; dx^T accumulators 12 tiles = 192 registers in the accumulator half, dy^T fragments 96 registers stationary) and
// per CHUNK of 32 hidden units (64 interleaved h1 | h3 columns):
//     dg^T [32 x 32]  = W2T_c [32 x 384] dy^T                      24 MFMAs        (W2T_c: six 32-row k-tile images in LDS)
//     dh1, dh3        = SwiGLU derivative against the saved h13 rows (one 16-byte load per lane and k16-step), rounded to bf16:
//                       the 8 values of a lane and step ARE the B fragment of the next product and the 16-byte dh13 store
//     dx^T [384 x 32] += W13T_c [384 x 64] dh13^T                  48 MFMAs        (W13T_c: one 384-row image in LDS)
// (Whole 128-token tiles take mlp_bwd_fused_asm_kernel further down: the same chain with its loop rotated by one product and the second
// product's step as a generated instruction stream.)
// The weight chunks (72 KB) arrive by LDS-DMA into a two-slot ring, chunk c + 1 requested when chunk c starts.  Products, operand
// slots and summation order are those of the two GEMM kernels this replaces (k in ascending 16-blocks), so dh13 and dx come out
// bit-identical to them (tests/test_kernels_gpu.py).
//
// Layout of this file: what the four kernels share is written once in front of them — the lane geometry and the image swizzle
// (LaneIds, swz_col), the stationary token fragments, the row-segment stores (row_segments, read_tile_rows, store_rows), the backward
// kernels' weight ring with its request offsets and slot addresses (BwdRing), their two products, SwiGLU derivative and dx epilogue, and
// the forward weight ring (FwdRing; mlp_up_fused_kernel keeps its own frame written out, for the measured reason given there).  The
// kernels keep the order of their requests and the counted waits that depend on it.
//
// Built WITHOUT -amdgpu-mfma-vgpr-form (frankenstein_amd/build.py): the 208 accumulator registers live in the AGPR half, which is what
// lets a wave keep 96 + 192 + 16 stationary registers at one wave per SIMD.
#include "fk_common.h"

namespace {

#include "gemm_tile.h"

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;
extern __shared__ __attribute__((aligned(16))) char smem[];      // the dynamic LDS of whichever kernel is running

struct MlpBwdArgs {
  const bf16_t* dy; const bf16_t* w2t; const bf16_t* h13; const bf16_t* w13t;
  bf16_t* dh13; bf16_t* dx;
  int64_t lddy, ldw2t, ldh, ldw13t, lddh, lddx;
  int M, H;
};

constexpr int MF_D = 384, MF_NW = 4, MF_TOK = MF_NW * 32;
constexpr int MF_KT = MF_D / 64;                          // k-tile images of a W2T chunk (6)
constexpr int MF_NT = MF_D / 32;                          // feature tiles of dx^T (12)
constexpr int MF_W2 = MF_KT * 32 * ROW_BYTES;            // 24 KiB
constexpr int MF_W13 = MF_D * ROW_BYTES;                 // 48 KiB
constexpr int MF_SLOT = MF_W2 + MF_W13;                  // 72 KiB
constexpr int MF_HREG = 32 * ROW_BYTES;                  // per wave: the 32 x 128-byte h13 / dh13 tile of a chunk (4 KiB)
constexpr int MF_LDS = 2 * MF_SLOT + MF_NW * MF_HREG;    // 160 KiB: the whole LDS of a CU
constexpr int MF_P2 = MF_W2 / 1024 / MF_NW;              // LDS-DMA wave instructions per wave and chunk: W2T part (6) ...
constexpr int MF_P13 = MF_W13 / 1024 / MF_NW;            // ... and W13T part (12)
constexpr int MF_ROWP = MF_D * 2 + 16;                   // padded bf16 row of the dx staging (784 B: 16-byte aligned, bank step 4)
static_assert(MF_LDS <= 160 * 1024 && MF_TOK * MF_ROWP <= MF_LDS, "LDS of a CU");
static_assert(MF_SLOT % (1024 * MF_NW) == 0, "whole pieces per wave");

template <bool FAST_SIGMOID> FK_DEV float mf_sigmoid(float x) {
  if constexpr (FAST_SIGMOID) return __builtin_amdgcn_rcpf(1.0f + __expf(-x));      // the bf16 mode's form in gemm.hip (sigmoid_f<bf16_t>)
  else return 1.0f / (1.0f + __expf(-x));
}

// One LDS-DMA request of 1 KiB (64 lanes x 16 B): wave-uniform 64-bit base + per-lane 32-bit byte offset -> LDS address `dst` (wave-uniform,
// through M0).  Issued as asm: the scalar-base form costs no address arithmetic per request (hipcc's builtin takes a per-lane 64-bit pointer:
// two or three VALU instructions per request on a wave that has no partner to hide them), and hipcc's wait-count pass does not see it
// (the waits are counted by hand in the kernels).  M0 is written one instruction ahead of its use.
FK_DEV void mf_dma(const void* base, unsigned voff, unsigned dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "s"(dst) : "memory");
}
FK_DEV void wait_all_barrier() { asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- the lane of all four kernels: token li of the wave's 32, k-half lh of a fragment; as a mover of 128-byte rows (LDS-DMA pieces, row
//      segment stores) it is 16-byte piece ch of row row8 of eight
struct LaneIds {
  int lane, li, lh, wave, row8, ch;
  FK_DEV LaneIds() {
    const int tid = threadIdx.x;
    lane = tid & 63, li = lane & 31, lh = lane >> 5;
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    row8 = lane >> 3, ch = lane & 7;
  }
};
// XOR swizzle of an NT image (nt_off) applied on the SOURCE side of a request: the column (in elements) whose 16-byte piece lands in place ch of image row r
FK_DEV int swz_col(int r, int ch) { return (ch ^ ((r >> 1) & 7)) << 3; }
FK_DEV unsigned row_byte_off(int row, int64_t ld, int col) { return (unsigned)(((int64_t)row * ld + col) * 2); }      // the launchers check 32 bits

// stationary B operand of a kernel's first product: the fragments of this lane's token row (k = 16 t + 8 lh .. + 8)
FK_DEV void load_token_frags(Frag<bf16_t> (&f)[MF_D / 16], const bf16_t* base, int row, int64_t ld, int lh) {
  const bf16_t* src = base + (int64_t)row * ld + 8 * lh;
#pragma unroll
  for (int t = 0; t < MF_D / 16; ++t) frag_load_contig<bf16_t>(f[t], src + 16 * t);
}
template <int N> FK_DEV void zero_acc(f32x16 (&a)[N]) {
#pragma unroll
  for (int t = 0; t < N; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) a[t][r] = 0.0f;
}

// ---- outputs leave as whole row segments: a wave-private LDS tile takes the lanes' pieces and is read back N rows-of-segments at a time
//      (per-lane row accesses, 16-byte pieces of 64 different rows per instruction, cost the backward kernel 190 us in loads and 530 us
//      in stores per cfg2 call).  Row j of a lane is row0 + j * step; rows past the end are clamped and never stored.
template <int N> FK_DEV void row_segments(bf16_t* (&dst)[N], bool (&ok)[N], bf16_t* base, int64_t ld, int row0, int step, int M, int col) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int mr = row0 + j * step;
    ok[j] = mr < M;
    dst[j] = base + (int64_t)(ok[j] ? mr : M - 1) * ld + col;
  }
}
// the 128-byte rows of a swizzled 32-row tile, eight lanes per row (LDS instructions of a wave execute in order: these reads see its own writes)
FK_DEV void read_tile_rows(bf16x8 (&rb)[4], const char* tile, const LaneIds& L) {
#pragma unroll
  for (int j = 0; j < 4; ++j) rb[j] = *reinterpret_cast<const bf16x8*>(tile + nt_off(j * 8 + L.row8, L.ch));
}
// whole wave (wave-uniform): no per-lane predicate and no branch per store; else per row
template <int N, bool NT> FK_DEV void store_rows(bf16_t* const (&dst)[N], const bool (&ok)[N], bool wave_full, int col, const bf16x8 (&v)[N]) {
  if (wave_full) {
#pragma unroll
    for (int j = 0; j < N; ++j) fk_st<NT>(reinterpret_cast<bf16x8*>(dst[j] + col), v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (ok[j]) fk_st<NT>(reinterpret_cast<bf16x8*>(dst[j] + col), v[j]);
  }
}

// ---- the backward kernels' weight ring.  LDS: W2T ring (two 24-KiB slots), W13T ring (two 48-KiB slots), the waves' h13 tiles.
//      LDS-DMA of one weight chunk: pieces of 8 image rows x 128 B (1 KiB per wave instruction); every wave moves six pieces of the W2T
//      part (k-tile images s6 = 0..5 of 32 rows each) and twelve of the 384-row W13T image; XOR swizzle on the SOURCE column.  The
//      per-lane byte offsets inside a chunk are constants: chunk c starts at w2t + c * 32 rows / w13t + c * 64 columns (wave-uniform).
//      The wave's h13 rows of a chunk (32 tokens x 64 interleaved columns = 4 KiB) also arrive by LDS-DMA, into a wave-private tile
//      with the image's swizzle; the lane reads its four 16-byte pieces from there, the dh13 pieces go back into the SAME places and
//      leave as whole 128-byte row segments.
struct BwdRing {
  const MlpBwdArgs& p;
  const LaneIds& L;
  unsigned lds0, off2[MF_P2], off13[MF_P13];
  FK_DEV BwdRing(const MlpBwdArgs& p_, const LaneIds& L_) : p(p_), L(L_), lds0((unsigned)(uintptr_t)(lds_void_t*)smem) {
#pragma unroll
    for (int j = 0; j < MF_P2; ++j) {
      const int q = L.wave * MF_P2 + j, s6 = q >> 2, r = (q & 3) * 8 + L.row8;
      off2[j] = (unsigned)((r * (int)p.ldw2t + s6 * 64 + swz_col(r, L.ch)) * 2);
    }
#pragma unroll
    for (int j = 0; j < MF_P13; ++j) {
      const int r = (L.wave * MF_P13 + j) * 8 + L.row8;
      off13[j] = (unsigned)((r * (int)p.ldw13t + swz_col(r, L.ch)) * 2);
    }
  }
  // the slots and this wave's tile (behind both weight rings), from base = smem (pointers) or lds0 (LDS byte addresses)
  template <typename B> static FK_DEV B w2_at(B base, int slot) { return base + slot * MF_W2; }
  template <typename B> static FK_DEV B w13_at(B base, int slot) { return base + 2 * MF_W2 + slot * MF_W13; }
  template <typename B> FK_DEV B tile_at(B base) const { return base + 2 * MF_SLOT + L.wave * MF_HREG; }
  FK_DEV const char* w2img(int slot) const { return w2_at(smem, slot); }
  FK_DEV const char* w13img(int slot) const { return w13_at(smem, slot); }
  FK_DEV char* tile() const { return tile_at(smem); }
  FK_DEV unsigned tile_lds() const { return __builtin_amdgcn_readfirstlane(tile_at(lds0)); }
  // source of chunk c (wave-uniform) and this wave's share of a slot as a request's LDS destination
  FK_DEV const bf16_t* w2_src(int c) const { return p.w2t + (int64_t)c * 32 * p.ldw2t; }
  FK_DEV const bf16_t* w13_src(int c) const { return p.w13t + (int64_t)c * 64; }
  FK_DEV const bf16_t* h_src(int c) const { return p.h13 + (int64_t)c * 64; }
  FK_DEV unsigned w2_dst(int slot) const { return __builtin_amdgcn_readfirstlane(w2_at(lds0, slot) + L.wave * (MF_W2 / MF_NW)); }
  FK_DEV unsigned w13_dst(int slot) const { return __builtin_amdgcn_readfirstlane(w13_at(lds0, slot) + L.wave * (MF_W13 / MF_NW)); }
  // one request (piece j of this wave's share) at a time: inside the chunk loops they are placed one behind each MFMA group, so that a wave
  // without a partner on its SIMD issues them in the shadow of its own matrix work instead of in bursts (-7 % per call, -0.44 ms per step)
  FK_DEV void dma_w2(int c, int slot, int j) const { mf_dma(w2_src(c), off2[j], w2_dst(slot) + j * 1024); }
  FK_DEV void dma_w13(int c, int slot, int j) const { mf_dma(w13_src(c), off13[j], w13_dst(slot) + j * 1024); }
  // tile request piece j (rows j * 8 + row8 of the tile): byte offset of token row `row` (the caller clamps it where M is ragged)
  FK_DEV unsigned h_off(int j, int row) const { return row_byte_off(row, p.ldh, swz_col(j * 8 + L.row8, L.ch)); }
  FK_DEV void dma_h(int c, int j, unsigned hoff, unsigned tile_dst) const { mf_dma(h_src(c), hoff, tile_dst + j * 1024); }
  // whole chunks, as the prologues request them
  FK_DEV void issue_w2(int c, int slot) const {
#pragma unroll
    for (int j = 0; j < MF_P2; ++j) dma_w2(c, slot, j);
  }
  FK_DEV void issue_w13(int c, int slot) const {
#pragma unroll
    for (int j = 0; j < MF_P13; ++j) dma_w13(c, slot, j);
  }
  FK_DEV void issue_h(int c, const unsigned (&hoff)[4], unsigned tile_dst) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) dma_h(c, j, hoff[j], tile_dst);
  }
};

// ---- dg^T = W2T_c dy^T: 24 MFMAs over MF_KT groups, the A fragments read one group (four) ahead (one wave per SIMD: nobody else hides the
//      LDS latency); behind(s6) is what the caller places behind group s6
template <typename F>
FK_DEV void first_product(f32x16& dg, Frag<bf16_t> (&fa)[2][4], const char* w2img, const Frag<bf16_t> (&dyf)[MF_D / 16], const LaneIds& L, const F& behind) {
#pragma unroll
  for (int r = 0; r < 16; ++r) dg[r] = 0.0f;
#pragma unroll
  for (int s = 0; s < 4; ++s) nt_frag<bf16_t>(fa[0][s], w2img, L.li, s, L.lh);
#pragma unroll
  for (int s6 = 0; s6 < MF_KT; ++s6) {
    if (s6 + 1 < MF_KT) {
#pragma unroll
      for (int s = 0; s < 4; ++s) nt_frag<bf16_t>(fa[(s6 + 1) & 1][s], w2img + (s6 + 1) * 32 * ROW_BYTES, L.li, s, L.lh);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) mma32<bf16_t>(dg, fa[s6 & 1][s], dyf[s6 * 4 + s]);
    behind(s6);
    // the next group's four LDS reads FIRST, then this group's four MFMAs (left alone hipcc puts the reads behind three of the MFMAs
    // and waits for them 32 cycles later)
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- SwiGLU derivative of one 16-byte h13 piece: lane (token, lh) holds dg of the hidden units 4 (2 s + lh) + e, e = 0..3, in dg[4 s + e];
//      the piece is (h1 | h3) of those four units, the result (dh1 | dh3) rounded to bf16
FK_DEV bf16x8 dswiglu_piece(const bf16x8& hv, const f32x16& dg, int s) {
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a1 = (float)hv[e], a3 = (float)hv[4 + e], g = dg[4 * s + e];
    const float sg = mf_sigmoid<true>(a1), ds = g * sg;
    o[e] = (bf16_t)(ds * a3 * (1.0f + a1 * (1.0f - sg)));
    o[4 + e] = (bf16_t)(ds * a1);
  }
  return o;
}

// ---- dx^T += W13T_c dh13^T: 48 MFMAs, fragments of feature tile t + 1 read while tile t multiplies; behind(t) is what the caller places
//      behind tile t
template <typename F>
FK_DEV void second_product(f32x16 (&dx)[MF_NT], Frag<bf16_t> (&fa)[2][4], const char* w13img, const Frag<bf16_t> (&bf)[4], const LaneIds& L, const F& behind) {
#pragma unroll
  for (int s = 0; s < 4; ++s) nt_frag<bf16_t>(fa[0][s], w13img, L.li, s, L.lh);
#pragma unroll
  for (int t = 0; t < MF_NT; ++t) {
    if (t + 1 < MF_NT) {
#pragma unroll
      for (int s = 0; s < 4; ++s) nt_frag<bf16_t>(fa[(t + 1) & 1][s], w13img, 32 * (t + 1) + L.li, s, L.lh);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) mma32<bf16_t>(dx[t], fa[t & 1][s], bf[s]);
    behind(t);
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- dx: accumulators (lane = token, 4 consecutive features per register group) -> padded bf16 rows staged in LDS (wave-private: the caller
//      has made sure the LDS is free) -> 16-byte row stores of the wave's rows m0w .. below row_end
FK_DEV void store_dx(const MlpBwdArgs& p, const f32x16 (&dx)[MF_NT], const LaneIds& L, int m0w, int row_end) {
  char* stg = smem + L.wave * 32 * MF_ROWP;
#pragma unroll
  for (int t = 0; t < MF_NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (bf16_t)dx[t][4 * g + e];
      *reinterpret_cast<bf16x4*>(stg + L.li * MF_ROWP + (32 * t + 8 * g + 4 * L.lh) * 2) = v;
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // wave-private staging: no barrier needed
  if (L.lane < MF_D / 8) {
    for (int r = 0; r < 32; ++r) {
      if (m0w + r >= row_end) break;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(stg + r * MF_ROWP + L.lane * 16);
      fk_st<true>(reinterpret_cast<bf16x8*>(p.dx + (int64_t)(m0w + r) * p.lddx + L.lane * 8), v);
    }
  }
}

#ifdef MF_STAMP
// diagnostic build only (tools/build_variant.py mf_stamp mlp_fused.hip -DMF_STAMP; tools/stamp_mlp.py): cycles per segment of a chunk, summed over
// waves.  s_memtime returns through lgkmcnt, so every stamp also drains the wave's LDS reads: coarse segments only.  Never in the product.
__device__ unsigned long long mf_stamp_acc[16];
#define MF_ST_DECL unsigned long long st_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long st_t = __builtin_amdgcn_s_memtime(); const unsigned long long st_t0 = st_t;
#define MF_ST(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[i] += t_ - st_t; st_t = t_; }
#define MF_ST_FLUSH(lane) if ((lane) == 0) { for (int i_ = 0; i_ < 10; ++i_) atomicAdd(&mf_stamp_acc[i_], st_acc[i_]); atomicAdd(&mf_stamp_acc[15], __builtin_amdgcn_s_memtime() - st_t0); }
#else
#define MF_ST_DECL
#define MF_ST(i)
#define MF_ST_FLUSH(lane)
#endif

// Ragged M (and dh13 blocks past 32-bit byte offsets): the chain as hipcc schedules it.
__global__ __launch_bounds__(MF_NW * 64, 1) void mlp_bwd_fused_kernel(MlpBwdArgs p) {
  using T = bf16_t;
  const LaneIds L;
  const BwdRing ring(p, L);
  const int m0w = blockIdx.x * MF_TOK + L.wave * 32, m = m0w + L.li;
  const int mc = m < p.M ? m : p.M - 1;                   // rows past the end: clamped loads, no stores
  const bool wave_full = m0w + 32 <= p.M;
  const int nchunks = p.H / 32, last = nchunks - 1;
  char* hreg = ring.tile();
  const unsigned hreg_lds = ring.tile_lds();
  T* hdst[4];                                             // dh13 store: logical piece ch of tile row j * 8 + row8
  bool hrow_ok[4];
  row_segments(hdst, hrow_ok, p.dh13, p.lddh, m0w + L.row8, 8, p.M, L.ch << 3);
  unsigned hoff[4];                                       // h13 tile request: the swizzled column piece of the same (clamped) rows
#pragma unroll
  for (int j = 0; j < 4; ++j) hoff[j] = ring.h_off(j, hrow_ok[j] ? m0w + j * 8 + L.row8 : p.M - 1);

  // ---- Request stream and waits.  Loads retire in order, so "s_waitcnt vmcnt(N)" with N = the number of YOUNGER loads of this wave says
  //      that a given request has landed (outstanding stores only make it wait longer, never less).  Per chunk c, per wave:
  //        B1(c): wait W2T(c), barrier   | request W13T(c + 1) [12]  | dg^T = W2T_c dy^T        | wait h13 tile(c) | SwiGLU', dh13 out [4 stores]
  //        B2(c): wait W13T(c), barrier  | request W2T(c + 2) [6], h13 tile(c + 1) [4]          | dx^T += W13T_c dh13^T
  //      so W2T is requested 1.6 chunks ahead of its use, W13T 1.4, the h13 tile one; the younger-load counts are
  //        at B1(c): tile(c-1) 4 + W13T(c) 12 + W2T(c+1) 6 + tile(c) 4 = 26;   before the SwiGLU': W13T(c+1) = 12;
  //        at B2(c): W2T(c+1) 6 + tile(c) 4 + W13T(c+1) 12 = 22.
  //      Past the last chunk the requests are repeated with the last chunk's addresses (into slots nobody reads any more), so that the
  //      counts hold to the end.
  ring.issue_w2(0, 0);
  ring.issue_w13(0, 0);
  ring.issue_w2(last < 1 ? last : 1, 1);
  ring.issue_h(0, hoff, hreg_lds);
  Frag<T> dyf[MF_D / 16];
  load_token_frags(dyf, p.dy, mc, p.lddy, L.lh);
  f32x16 dx[MF_NT];
  zero_acc(dx);
  wait_all_barrier();                                     // B1(0): everything requested so far (and the dy fragments) has landed

  for (int c = 0; c < nchunks; ++c) {
    if (c > 0) asm volatile("s_waitcnt vmcnt(26)\n\ts_barrier" ::: "memory");              // B1(c)
    const int cn1 = c + 1 < nchunks ? c + 1 : last, cn2 = c + 2 < nchunks ? c + 2 : last;
    f32x16 dg;
    Frag<T> fa[2][4];
    // W13T(c + 1): two of this wave's twelve requests behind each of the six groups (that slot was last read by the second product of chunk c - 1)
    first_product(dg, fa, ring.w2img(c & 1), dyf, L, [&](int s6) __attribute__((always_inline)) {
      ring.dma_w13(cn1, (c + 1) & 1, 2 * s6);
      ring.dma_w13(cn1, (c + 1) & 1, 2 * s6 + 1);
    });
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");       // this wave's h13 tile of chunk c has landed (wave-private: no barrier)
    Frag<T> bf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf[s].v = dswiglu_piece(*reinterpret_cast<const bf16x8*>(hreg + nt_off(L.li, 2 * s + L.lh)), dg, s);
      *reinterpret_cast<bf16x8*>(hreg + nt_off(L.li, 2 * s + L.lh)) = bf[s].v;       // the place this lane just read
    }
    // dh13 leaves as whole row segments: read back here, stored behind the barrier so that the LDS latency hides in the wait
    bf16x8 rb[4];
    read_tile_rows(rb, hreg, L);
    asm volatile("s_waitcnt vmcnt(22)\n\ts_barrier" ::: "memory");               // B2(c): W13T(c) has landed; everyone is done with W2T(c)
    store_rows<4, true>(hdst, hrow_ok, wave_full, c * 64, rb);                   // written once, read by the weight-gradient GEMMs later
    // W2T(c + 2) behind the first six tiles, then the h13 tile of chunk c + 1 (free: its read-back sits in registers)
    second_product(dx, fa, ring.w13img(c & 1), bf, L, [&](int t) __attribute__((always_inline)) {
      if (t < MF_P2) ring.dma_w2(cn2, c & 1, t);
      else if (t < MF_P2 + 4) ring.dma_h(cn1, t - MF_P2, hoff[t - MF_P2], hreg_lds);
    });
  }
  wait_all_barrier();                                     // the repeated requests of the tail have landed: the LDS is free for the dx staging
  store_dx(p, dx, L, m0w, p.M);
}


// ================================================================================================================================
// The same chain with its loop rotated by one product and the second product's step as a GENERATED instruction stream (round 4).
//   A wave of mlp_bwd_fused_kernel is alone on its SIMD, so everything it issues shares one in-order stream, and the stamps
//   (tools/stamp_mlp.py, profiles/r04_mf_stamps*.txt) fit one model: a gap behind an MFMA costs max(32, 8 + the issue time of what is
//   placed in it) cycles.  The kernel above spends ~1900 cycles per chunk in the SwiGLU derivative with the matrix pipe idle (32 % of a
//   wave's life); hipcc asked to interleave puts 8-9 VALU with two transcendentals into 32 of the 48 gaps of the second product (64
//   cycles each) and leaves the rest at 32: no gain.  Here iteration c runs
//        A(c): dg^T(c + 1) = W2T_{c+1} dy^T                      24 MFMAs (hipcc), the W13T(c + 1) requests behind its groups
//        B(c): dx^T += W13T_c dh13^T(c)  BESIDE  the SwiGLU derivative of chunk c + 1, its dh13 tile round trip and stores, the W2T(c + 3)
//              and h13 tile(c + 2) requests, the barrier         48 MFMAs: mlpb_step_asm (tools/gen/gen_mlpb_asm.py -> mlp_bwd_asm.inc),
//              every gap filled to the same issue budget
//   Same products and summation order, same arithmetic instruction for instruction: dh13 and dx are the bits of the kernel above.
//   Whole 128-token tiles only (M % 128 == 0); the launcher keeps the kernel above for the rest.
//   The prologue (chunk 0's first product and derivative) and the tail (the last chunk's second product, the dx epilogue) are the shared
//   blocks above; A(c) is written out here, because barrier B(c) and the stream's first operands sit INSIDE its last group.
//
//   Requests and waits (loads retire in order; N = the younger loads of this wave).  Issue order per wave:
//        A(c): W13T(c + 1) [12]      B(c): W2T(c + 3) [6], dh13(c + 1) stores, h13 tile(c + 2) [4]      A(c + 1): W13T(c + 2) [12] ...
//   * barrier B(c), in front of the last MFMA group of A(c): needs W13T(c) and this wave's tile(c + 1); the youngest loads are the 10
//     W13T(c + 1) requests issued so far -> vmcnt(10); everything older has landed then, W2T(c + 2) included.  Behind it the W2T slot of
//     chunk c + 1 is free (-> W2T(c + 3)), and the caller reads the stream's first fragments and its h13 pieces under the last MFMAs.
//   * barrier A(c + 1), inside the stream in front of its last four MFMAs: nothing to wait for but this wave's own fragment reads; behind
//     it the W13T slot of chunk c is free for the W13T(c + 2) requests of A(c + 1), whose first fragments the stream reads on its way out.
typedef unsigned u32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
#ifndef FK_MLPB_INC
#define FK_MLPB_INC "mlp_bwd_asm.inc"
#endif
#include FK_MLPB_INC

__global__ __launch_bounds__(MF_NW * 64, 1) void mlp_bwd_fused_asm_kernel(MlpBwdArgs p) {
  MF_ST_DECL
  using T = bf16_t;
  const LaneIds L;
  const BwdRing ring(p, L);
  const int m0w = blockIdx.x * MF_TOK + L.wave * 32;        // + li < M: whole tiles only
  const int nchunks = p.H / 32, last = nchunks - 1;
  auto cl = [&](int k) { return k < last ? k : last; };
  char* hreg = ring.tile();
  const unsigned hreg_lds = ring.tile_lds();
  // the stream's address operands: LDS byte addresses (adr) and global byte offsets (ofs); adr[0..3] and adr[12..15] follow the ring slots
  u32x16 adr, ofs;
  unsigned ax[4], hoff[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    ax[s] = (unsigned)nt_off(L.li, 2 * s + L.lh);
    adr[4 + s] = hreg_lds + ax[s];                                          // AH: the lane's pieces of its tile
    adr[8 + s] = hreg_lds + (unsigned)nt_off(s * 8 + L.row8, L.ch);         // AR: tile rows, eight lanes per row
  }
#pragma unroll
  for (int j = 0; j < MF_P2; ++j) ofs[j] = ring.off2[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hoff[j] = ring.h_off(j, m0w + j * 8 + L.row8);
    ofs[6 + j] = hoff[j];                                                                        // HOFF: tile request pieces (swizzled source column)
    ofs[10 + j] = row_byte_off(m0w + j * 8 + L.row8, p.lddh, L.ch << 3);                        // VST: row stores (logical piece ch of row r)
  }
  ofs[14] = 0;
  ofs[15] = 0;

  // ---- prologue: W2T(0), W13T(0), W2T(1), tile(0); dy^T fragments; chunk 0's first product and SwiGLU derivative alone
  ring.issue_w2(0, 0);
  ring.issue_w13(0, 0);
  ring.issue_w2(cl(1), 1);
  ring.issue_h(0, hoff, hreg_lds);
  Frag<T> dyf[MF_D / 16];
  load_token_frags(dyf, p.dy, m0w + L.li, p.lddy, L.lh);
  f32x16 dx[MF_NT];
  zero_acc(dx);
  MF_ST(4)                                                  // (stamp build: requests issued, dy fragments requested)
  wait_all_barrier();
  MF_ST(5)                                                  // (stamp build: the first wait)
  Frag<T> fa[2][4];
  f32x16 dg;
  u32x16 fa0, bfc, bfn, hvv;
  first_product(dg, fa, ring.w2img(0), dyf, L, [](int) {});
  {
    bf16x8 rb[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 o = dswiglu_piece(*reinterpret_cast<const bf16x8*>(hreg + nt_off(L.li, 2 * s + L.lh)), dg, s);
      *reinterpret_cast<bf16x8*>(hreg + nt_off(L.li, 2 * s + L.lh)) = o;
      const u32x4v w = __builtin_bit_cast(u32x4v, o);
#pragma unroll
      for (int k = 0; k < 4; ++k) bfc[4 * s + k] = w[k];
    }
    read_tile_rows(rb, hreg, L);
#pragma unroll
    for (int j = 0; j < 4; ++j)                             // whole tiles: no row is past the end; non-temporal like every dh13 store
      fk_st<true>(reinterpret_cast<bf16x8*>(p.dh13 + (int64_t)(m0w + j * 8 + L.row8) * p.lddh + (L.ch << 3)), rb[j]);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");    // everyone is done with W2T(0); this wave's tile rows are in registers
  ring.issue_w2(cl(2), 0);
  ring.issue_h(cl(1), hoff, hreg_lds);
#pragma unroll
  for (int s = 0; s < 4; ++s) {                                       // A(0)'s first fragments: W2T(1) landed in front of the first barrier
    const u32x4v w = *reinterpret_cast<const u32x4v*>(ring.w2img(1) + ax[s]);
#pragma unroll
    for (int k = 0; k < 4; ++k) fa0[4 * s + k] = w[k];
  }

  MF_ST(0)                                                  // prologue
  for (int c = 0; c < last; ++c) {
    const char* w2img = ring.w2img((c + 1) & 1);
    const char* w13img = ring.w13img(c & 1);
    // ---- A(c): dg^T(c + 1), 24 MFMAs, fragments one group ahead; the last group behind barrier B(c)
#pragma unroll
    for (int r = 0; r < 16; ++r) dg[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const u32x4v w = {fa0[4 * s], fa0[4 * s + 1], fa0[4 * s + 2], fa0[4 * s + 3]};
      fa[0][s].v = __builtin_bit_cast(bf16x8, w);
    }
#pragma unroll
    for (int s6 = 0; s6 < MF_KT; ++s6) {
      if (s6 + 1 < MF_KT) {
#pragma unroll
        for (int s = 0; s < 4; ++s) nt_frag<T>(fa[(s6 + 1) & 1][s], w2img + (s6 + 1) * 32 * ROW_BYTES, L.li, s, L.lh);
      } else {
        __builtin_amdgcn_sched_barrier(0);
        MF_ST(1)                                            // first product, groups 0-4
        asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)\n\ts_barrier" ::: "memory");        // barrier B(c)
        MF_ST(2)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const u32x4v w = *reinterpret_cast<const u32x4v*>(w13img + ax[s]);             // the stream's first fragments (feature tile 0) ...
          const u32x4v h = *reinterpret_cast<const u32x4v*>(hreg + ax[s]);               // ... and this wave's h13 pieces of chunk c + 1
#pragma unroll
          for (int k = 0; k < 4; ++k) { fa0[4 * s + k] = w[k]; hvv[4 * s + k] = h[k]; }
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) mma32<T>(dg, fa[s6 & 1][s], dyf[s6 * 4 + s]);
      ring.dma_w13(cl(c + 1), (c + 1) & 1, 2 * s6);
      ring.dma_w13(cl(c + 1), (c + 1) & 1, 2 * s6 + 1);
      if (s6 + 1 < MF_KT) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      else __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    MF_ST(3)                                                // group 5
    // ---- B(c): the generated step
    const unsigned w13a = ring.w13_at(ring.lds0, c & 1), w2a = ring.w2_at(ring.lds0, c & 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      adr[s] = w13a + ax[s];
      adr[12 + s] = w2a + ax[s];
    }
    mlpb_step_asm(dx, dg, fa0, bfc, bfn, hvv, adr, ofs, ring.w2_src(cl(c + 3)), ring.h_src(cl(c + 2)), p.dh13 + (int64_t)(c + 1) * 64,
                  ring.w2_dst((c + 1) & 1), hreg_lds);
    bfc = bfn;
    MF_ST(6)                                                // the generated step (barrier A inside)
  }
  // ---- the last chunk's second product, alone
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");     // W13T(last) and the repeated requests of the tail have landed
  MF_ST(7)
  {
    Frag<T> bf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const u32x4v w = {bfc[4 * s], bfc[4 * s + 1], bfc[4 * s + 2], bfc[4 * s + 3]};
      bf[s].v = __builtin_bit_cast(bf16x8, w);
    }
    second_product(dx, fa, ring.w13img(last & 1), bf, L, [](int) {});
  }
  MF_ST(8)                                                  // the last chunk's second product
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // every wave has its last fragments: the LDS is free for the dx staging
  store_dx(p, dx, L, m0w, m0w + 32);
  MF_ST(9)                                                  // dx epilogue
  MF_ST_FLUSH(L.lane)
}


// ================================================================================================================================
// The forward up-projection + SwiGLU of the same MLP with the token on the lane (what fk_gemm_nt_swiglu computes: H13 and G).
//   Per wave 32 tokens with x^T stationary (96 registers); per chunk of 32 hidden units the W13 rows arrive as TWO 32-row tiles — tile 0
//   the h1 rows, tile 1 the h3 rows of the same units — so that a lane finds h1 and h3 of a unit in the same register index of its two
//   accumulators and silu(h1) * h3 happens in registers, without the fp32 staging sweep of the tiled kernel.  No accumulator outlives a
//   chunk, so a wave needs ~200 registers: two waves per SIMD, eight per workgroup (256 tokens), and the weight chunk (48 KiB) is shared by
//   twice as many tokens as in the backward kernel above.  h13 (16 bytes per lane and k-group) and g (8 bytes) leave through wave-private LDS
//   tiles as whole row segments; the stores of chunk c are issued at the head of chunk c + 1 (from registers), i.e. BEFORE the next weight
//   request, so that the end-of-chunk wait finds only requests that are a whole chunk old.  Same products and summation order as
//   gemm_nt_ring2_kernel<.., 1>: bit-identical H13 and G.
//   This kernel keeps its frame WRITTEN OUT (its own lane ids, request offsets, issue_w, row segments and stores) although
//   qkv_rope_fused_kernel below has the same frame from LaneIds / FwdRing / row_segments / store_rows: hipcc's schedule of the chunk loop
//   (where the exponentials and reciprocals of the SwiGLU land between the other VALU work) and its register assignment move with any of
//   them, and every shared form measured 1.5-2.5 % slower at the cfg2 shape (536-545 us against 526-533; the numbers:
//   profiles/mlp_fused_shared_scaffolding_ab.txt) — also the one whose chunk loop is the same instruction sequence.  As written it
//   compiles to the code it has always had; whoever next changes its schedule on purpose can move it onto FwdRing in the same step.
struct MlpUpArgs {
  const bf16_t* x; const bf16_t* w13; bf16_t* h13; bf16_t* g;
  int64_t ldx, ldw, ldh, ldg;
  int M, H;
};
constexpr int MU_NW = 8, MU_TOK = MU_NW * 32;
constexpr int MU_TILE = MF_KT * 32 * ROW_BYTES;          // one 32-row tile of a chunk: six k-tile images (24 KiB)
constexpr int MU_SLOT = 2 * MU_TILE;                     // two tiles (48 KiB)
constexpr int MU_HT = 32 * ROW_BYTES, MU_GT = 32 * 64;   // per wave: h13 tile (32 x 128 B), g tile (32 x 64 B)
constexpr int MU_LDS = 2 * MU_SLOT + MU_NW * (MU_HT + MU_GT);
static_assert(MU_LDS <= 160 * 1024, "LDS of a CU");
constexpr int MU_PIECES = MU_SLOT / 1024 / MU_NW;        // 6 requests per wave and chunk

// ---- the forward kernels' weight ring (qkv_rope_fused_kernel; mlp_up_fused_kernel has the same, written out: see there): two slots of
//      two 32-row tiles each, a chunk = 64 weight rows.  Piece q = wave * 6 + j of a slot is
//      tile q / 24, k-tile image (q % 24) >> 2, image rows (q & 3) * 8 + row8; wrow(tile, n) says which of the chunk's 64 weight rows image
//      row n of that tile is.
struct FwdRing {
  const bf16_t* w;
  int64_t ldw;
  unsigned lds0, woff[MU_PIECES];
  int wave;
  template <typename RowMap> FK_DEV FwdRing(const bf16_t* w_, int64_t ldw_, const LaneIds& L, const RowMap& wrow) : w(w_), ldw(ldw_), lds0((unsigned)(uintptr_t)(lds_void_t*)smem), wave(L.wave) {
#pragma unroll
    for (int j = 0; j < MU_PIECES; ++j) {
      const int q = L.wave * MU_PIECES + j, tile = q / 24, s6 = (q % 24) >> 2, n = (q & 3) * 8 + L.row8;
      woff[j] = (unsigned)((wrow(tile, n) * (int)ldw + s6 * 64 + swz_col(n, L.ch)) * 2);
    }
  }
  FK_DEV void issue_w(int c, int slot) const {
    const void* gw = w + (int64_t)c * 64 * ldw;
    const unsigned d = __builtin_amdgcn_readfirstlane(lds0 + slot * MU_SLOT + wave * (MU_SLOT / MU_NW));      // this wave's share of the slot
#pragma unroll
    for (int j = 0; j < MU_PIECES; ++j) mf_dma(gw, woff[j], d + j * 1024);
  }
};

__global__ __launch_bounds__(MU_NW * 64, 2) void mlp_up_fused_kernel(MlpUpArgs p) {
  using T = bf16_t;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0w = blockIdx.x * MU_TOK + wave * 32;
  const int m = m0w + li, mc = m < p.M ? m : p.M - 1;
  const bool wave_full = m0w + 32 <= p.M;
  const int nchunks = p.H / 32, last = nchunks - 1;
  const int row8 = lane >> 3, ch = lane & 7;
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_void_t*)smem;

  // requests: piece q = wave * 6 + j of the slot: tile q / 24 (0: h1 rows, 1: h3 rows), k-tile image (q % 24) >> 2, image rows (q & 3) * 8 + row8.
  // Image row n of a tile is hidden unit 32 c + n: interleaved W13 row 8 (n / 4) + n % 4 (+ 4 for h3) of the chunk's 64 rows.
  unsigned woff[MU_PIECES];
#pragma unroll
  for (int j = 0; j < MU_PIECES; ++j) {
    const int q = wave * MU_PIECES + j, tile = q / 24, s6 = (q % 24) >> 2, n = (q & 3) * 8 + row8;
    const int wrow = 8 * (n >> 2) + (n & 3) + 4 * tile;
    woff[j] = (unsigned)((wrow * (int)p.ldw + s6 * 64 + swz_col(n, ch)) * 2);
  }
  auto issue_w = [&](int c, int slot) __attribute__((always_inline)) {
    const void* gw = p.w13 + (int64_t)c * 64 * p.ldw;
    const unsigned d0 = __builtin_amdgcn_readfirstlane(lds0 + slot * MU_SLOT + wave * (MU_SLOT / MU_NW));
#pragma unroll
    for (int j = 0; j < MU_PIECES; ++j) mf_dma(gw, woff[j], d0 + j * 1024);
  };
  char* htile = smem + 2 * MU_SLOT + wave * (MU_HT + MU_GT);
  char* gtile = htile + MU_HT;
  // output rows of the read-back: h13 eight lanes per row (8 rows per instruction), g four lanes per row (16 rows per instruction)
  T* hdst[4];
  T* gdst[2];
  bool hok[4], gok[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int mr = m0w + j * 8 + row8;
    hok[j] = mr < p.M;
    hdst[j] = p.h13 + (int64_t)(hok[j] ? mr : p.M - 1) * p.ldh + (ch << 3);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int mr = m0w + j * 16 + (lane >> 2);
    gok[j] = mr < p.M;
    gdst[j] = p.g + (int64_t)(gok[j] ? mr : p.M - 1) * p.ldg + ((lane & 3) << 3);
  }

  issue_w(0, 0);
  Frag<T> xf[MF_D / 16];
  const T* xrow = p.x + (int64_t)mc * p.ldx + 8 * lh;
#pragma unroll
  for (int t = 0; t < MF_D / 16; ++t) frag_load_contig<T>(xf[t], xrow + 16 * t);
  wait_all_barrier();     // chunk 0 and the x fragments have landed

  bf16x8 rbh[4] = {}, rbg[2] = {};
  for (int c = 0; c < nchunks; ++c) {
    const char* t0 = smem + (c & 1) * MU_SLOT;
    const char* t1 = t0 + MU_TILE;
    // the previous chunk's outputs (in registers since its read-back), then the next chunk's weights: the wait at the end of THIS chunk then
    // only covers requests issued a whole chunk earlier
    if (c > 0) {
      if (wave_full) {
#pragma unroll
        for (int j = 0; j < 4; ++j) fk_st<true>(reinterpret_cast<bf16x8*>(hdst[j] + (c - 1) * 64), rbh[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) fk_st<true>(reinterpret_cast<bf16x8*>(gdst[j] + (c - 1) * 32), rbg[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (hok[j]) fk_st<true>(reinterpret_cast<bf16x8*>(hdst[j] + (c - 1) * 64), rbh[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (gok[j]) fk_st<true>(reinterpret_cast<bf16x8*>(gdst[j] + (c - 1) * 32), rbg[j]);
      }
    }
    issue_w(c + 1 < nchunks ? c + 1 : last, (c + 1) & 1);          // that slot was read in chunk c - 1: every wave is past the barrier behind it
    // ---- H^T = W13_c x^T: two accumulator tiles (h1 rows, h3 rows of the same 32 units), 48 MFMAs, fragments read one k-tile ahead
    f32x16 a1, a3;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a1[r] = 0.0f; a3[r] = 0.0f; }
    Frag<T> f1[2][4], f3[2][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { nt_frag<T>(f1[0][s], t0, li, s, lh); nt_frag<T>(f3[0][s], t1, li, s, lh); }
#pragma unroll
    for (int s6 = 0; s6 < MF_KT; ++s6) {
      if (s6 + 1 < MF_KT) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          nt_frag<T>(f1[(s6 + 1) & 1][s], t0 + (s6 + 1) * 32 * ROW_BYTES, li, s, lh);
          nt_frag<T>(f3[(s6 + 1) & 1][s], t1 + (s6 + 1) * 32 * ROW_BYTES, li, s, lh);
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        mma32<T>(a1, f1[s6 & 1][s], xf[s6 * 4 + s]);
        mma32<T>(a3, f3[s6 & 1][s], xf[s6 * 4 + s]);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- SwiGLU in registers: accumulator register 4 g + i of lane (token, lh) is hidden unit 8 g + 4 lh + i of the chunk in BOTH tiles;
    //      the four units of a register group are interleaved hidden group 2 g + lh: one 16-byte piece of h13, one 8-byte piece of g
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x8 hp;
      bf16x4 gp;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float h1 = a1[4 * g4 + i], h3 = a3[4 * g4 + i];
        hp[i] = (T)h1;
        hp[4 + i] = (T)h3;
        gp[i] = (T)(h1 * mf_sigmoid<true>(h1) * h3);
      }
      const int q = 2 * g4 + lh;
      *reinterpret_cast<bf16x8*>(htile + nt_off(li, q)) = hp;
      *reinterpret_cast<bf16x4*>(gtile + li * 64 + ((((q >> 1) + li) & 3) << 4) + ((q & 1) << 3)) = gp;      // 16-byte chunks rotated by the row
    }
    // read back as whole row segments (LDS instructions of a wave execute in order); stored at the head of the next chunk
#pragma unroll
    for (int j = 0; j < 4; ++j) rbh[j] = *reinterpret_cast<const bf16x8*>(htile + nt_off(j * 8 + row8, ch));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = j * 16 + (lane >> 2);
      rbg[j] = *reinterpret_cast<const bf16x8*>(gtile + r * 64 + ((((lane & 3) + r) & 3) << 4));
    }
    wait_all_barrier();   // chunk c + 1 has landed (requested a chunk ago, like the stores in front of it); everyone is done with this slot
  }
  if (wave_full) {
#pragma unroll
    for (int j = 0; j < 4; ++j) fk_st<true>(reinterpret_cast<bf16x8*>(hdst[j] + last * 64), rbh[j]);
#pragma unroll
    for (int j = 0; j < 2; ++j) fk_st<true>(reinterpret_cast<bf16x8*>(gdst[j] + last * 32), rbg[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (hok[j]) fk_st<true>(reinterpret_cast<bf16x8*>(hdst[j] + last * 64), rbh[j]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (gok[j]) fk_st<true>(reinterpret_cast<bf16x8*>(gdst[j] + last * 32), rbg[j]);
  }
}


// ================================================================================================================================
// The packed q | k | v projection with fused RoPE and pre-scaled queries (what fk_gemm_nt_rope computes) with the token on the lane.
//   The frame of mlp_up_fused_kernel, from the shared blocks (FwdRing, the stationary x^T, the row-segment stores): two waves per SIMD, a chunk = 64 output
//   columns = ONE head (two 32-column accumulator tiles), no accumulator outlives a chunk.  A lane owns 4 consecutive columns per register
//   group = two complex pairs, so the rotation is register arithmetic; its (cos, sin) pairs — 16 bytes per register group, 8 groups per chunk, from the lane's own token row
//   of the L2-resident table (the pre-scaled copy for the query heads) — are requested at the head of the chunk, in front of the next
//   weight request, and waited for with a counted vmcnt (loads retire in order: 6 younger requests).  Same products, summation order and
//   rotation arithmetic as gemm_nt_ring2_kernel<.., 3>: bit-identical output.
struct QkvArgs {
  const bf16_t* x; const bf16_t* w; bf16_t* out; const float* table;
  int64_t ldx, ldw, ldo, table_bs, q_off;
  int M, N, T, pos_off, rot_chunks, q_chunks;
};
constexpr int QK_LDS = 2 * MU_SLOT + MU_NW * MU_HT;
static_assert(QK_LDS <= 160 * 1024, "LDS of a CU");

__global__ __launch_bounds__(MU_NW * 64, 2) void qkv_rope_fused_kernel(QkvArgs p) {
  using T = bf16_t;
  const LaneIds L;
  const int lh = L.lh;
  const int m0w = blockIdx.x * MU_TOK + L.wave * 32;
  const int m = m0w + L.li, mc = m < p.M ? m : p.M - 1;
  const bool wave_full = m0w + 32 <= p.M;
  const int nchunks = p.N / 64, last = nchunks - 1;
  // tile 0 / 1: columns 0..31 / 32..63 of the head, image row n = column 32 tile + n
  const FwdRing ring(p.w, p.ldw, L, [](int tile, int n) { return 32 * tile + n; });
  char* htile = smem + 2 * MU_SLOT + L.wave * MU_HT;
  T* odst[4];
  bool ook[4];
  row_segments(odst, ook, p.out, p.ldo, m0w + L.row8, 8, p.M, L.ch << 3);
  // this lane's (cos, sin) row: token mc is position pos_off + mc % T of sample mc / T; the lane's pairs start at pair 2 lh (4 floats per piece)
  const float* trow = p.table + (int64_t)(mc / p.T) * p.table_bs + (int64_t)(p.pos_off + mc % p.T) * 64 + 4 * lh;

  ring.issue_w(0, 0);
  Frag<T> xf[MF_D / 16];
  load_token_frags(xf, p.x, mc, p.ldx, lh);
  wait_all_barrier();                                     // chunk 0 and the x fragments have landed

  bf16x8 rb[4] = {};
  for (int c = 0; c < nchunks; ++c) {
    const char* t0 = smem + (c & 1) * MU_SLOT;
    const char* t1 = t0 + MU_TILE;
    if (c > 0) store_rows<4, true>(odst, ook, wave_full, (c - 1) * 64, rb);      // the previous head's rows (in registers since its read-back)
    const bool rot = c < p.rot_chunks;                    // workgroup-uniform
    f32x4 cs[8];
    if (rot) {
      const float* tq = trow + (c < p.q_chunks ? p.q_off : (int64_t)0);
      asm volatile("global_load_dwordx4 %0, %8, off\n\tglobal_load_dwordx4 %1, %8, off offset:32\n\t"
                   "global_load_dwordx4 %2, %8, off offset:64\n\tglobal_load_dwordx4 %3, %8, off offset:96\n\t"
                   "global_load_dwordx4 %4, %8, off offset:128\n\tglobal_load_dwordx4 %5, %8, off offset:160\n\t"
                   "global_load_dwordx4 %6, %8, off offset:192\n\tglobal_load_dwordx4 %7, %8, off offset:224"
                   : "=&v"(cs[0]), "=&v"(cs[1]), "=&v"(cs[2]), "=&v"(cs[3]), "=&v"(cs[4]), "=&v"(cs[5]), "=&v"(cs[6]), "=&v"(cs[7])
                   : "v"(tq) : "memory");
    }
    ring.issue_w(c + 1 < nchunks ? c + 1 : last, (c + 1) & 1);     // that slot was read in chunk c - 1: every wave is past the barrier behind it
    // ---- two accumulator tiles of the head: 48 MFMAs, four fragments read ahead (tile 0 and tile 1 of a k-tile alternate)
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.0f; acc[1][r] = 0.0f; }
    Frag<T> f[2][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) nt_frag<T>(f[0][s], t0, L.li, s, lh);
#pragma unroll
    for (int gq = 0; gq < 2 * MF_KT; ++gq) {               // group gq: tile gq & 1 of k-tile gq >> 1
      if (gq + 1 < 2 * MF_KT) {
        const char* nx = ((gq + 1) & 1 ? t1 : t0) + ((gq + 1) >> 1) * 32 * ROW_BYTES;
#pragma unroll
        for (int s = 0; s < 4; ++s) nt_frag<T>(f[(gq + 1) & 1][s], nx, L.li, s, lh);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) mma32<T>(acc[gq & 1], f[gq & 1][s], xf[(gq >> 1) * 4 + s]);
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (rot)      // the (cos, sin) pieces have landed: six younger requests (the next weight chunk) may still be in flight
      asm volatile("s_waitcnt vmcnt(6)" : "+v"(cs[0]), "+v"(cs[1]), "+v"(cs[2]), "+v"(cs[3]), "+v"(cs[4]), "+v"(cs[5]), "+v"(cs[6]), "+v"(cs[7])::"memory");
    // ---- rotation in registers (the arithmetic of nt_epilogue's fused RoPE: explicit fma shape), rounding, 8-byte pieces into the row tile
#pragma unroll
    for (int tl = 0; tl < 2; ++tl)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float v[4] = {acc[tl][4 * g4], acc[tl][4 * g4 + 1], acc[tl][4 * g4 + 2], acc[tl][4 * g4 + 3]};
        if (rot) {
          const f32x4 t = cs[4 * tl + g4];                 // (c0, s0, c1, s1) of the pairs 16 tl + 4 g4 + 2 lh, + 1
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float re = v[2 * j], im = v[2 * j + 1];
            v[2 * j] = __builtin_fmaf(re, t[2 * j], -(im * t[2 * j + 1]));
            v[2 * j + 1] = __builtin_fmaf(re, t[2 * j + 1], im * t[2 * j]);
          }
        }
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
        *reinterpret_cast<bf16x4*>(htile + nt_off(L.li, 4 * tl + g4) + 8 * lh) = o;
      }
    read_tile_rows(rb, htile, L);
    wait_all_barrier();                                   // chunk c + 1 has landed (requested a chunk ago); everyone is done with this slot
  }
  store_rows<4, true>(odst, ook, wave_full, last * 64, rb);
}

}  // namespace

// the token-on-the-lane form of fk_gemm_nt_rope (called from gemm.hip's entry point)
// One 8-wave workgroup of 256 tokens per CU at a time: the launch runs in rounds of 256 workgroups, so its time is a step function of M
// (150 / 293 / 460 us at <= 65 536 / 131 072 / 196 608 rows for the up-projection) where the tiled kernels' is linear.  Measured over
// M = 19 200 ... 196 608 (profiles/r04_mlp_size_sweep.txt): these kernels win wherever the last round is at least
// ~40 % full, i.e. the grid fills >= 70 % of its rounds (49 152: 0.75 wins; 38 400 and 76 800: 0.59 lose by 5-12 %).
static bool mu_grid_fills(int64_t M) {
  const int64_t wg = fk_cdiv(M, MU_TOK), rounds = fk_cdiv(wg, 256);
  return wg * 10 >= rounds * 256 * 7;
}
bool fk_qkv_rope_fused_ok(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, bool has_bias, int64_t T, int64_t D, int64_t rot_cols,
                          int64_t q_cols, int dtype) {
  // anything launch_nt would refuse (an empty problem, a leading dimension shorter than its row) is left to it: this kernel has no checks of its own
  return dtype == FK_BF16 && K == MF_D && D == 64 && N > 0 && N < (1LL << 31) && N % 64 == 0 && rot_cols % 64 == 0 && q_cols % 64 == 0 && rot_cols <= N && !has_bias &&
         mu_grid_fills(M) && M < (1LL << 31) && T > 0 && M % T == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && lda >= K && ldb >= K && ldc >= N &&
         64 * ldb * 2 < (1LL << 32);
}
int fk_qkv_rope_fused_launch(const void* A, int64_t lda, const void* W, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, const float* table,
                             int64_t table_bs, int64_t T, int64_t pos_off, int64_t rot_cols, int64_t q_cols, int64_t q_off, void* stream) {
  QkvArgs a{(const bf16_t*)A, (const bf16_t*)W, (bf16_t*)C, table, lda, ldb, ldc, table_bs, q_off, (int)M, (int)N, (int)T, (int)pos_off,
            (int)(rot_cols / 64), (int)(q_cols / 64)};
  fk_launch_lds<qkv_rope_fused_kernel>(dim3((unsigned)fk_cdiv(M, MU_TOK)), dim3(MU_NW * 64), QK_LDS, (hipStream_t)stream, a);
  FK_CHECK_LAUNCH("fk_gemm_nt_rope (token-on-the-lane kernel)");
  return FK_OK;
}

// the token-on-the-lane form of fk_gemm_nt_swiglu for the shapes it is built for (called from gemm.hip's entry point)
bool fk_mlp_up_fused_ok(int64_t M, int64_t H, int64_t K, int64_t lda, int64_t ldb, int64_t ldh, int64_t ldg, int dtype) {
  return dtype == FK_BF16 && K == MF_D && H > 0 && H < (1LL << 30) && H % 32 == 0 && mu_grid_fills(M) && M < (1LL << 31) && lda % 8 == 0 && ldb % 8 == 0 &&
         ldh % 8 == 0 && ldg % 8 == 0 && lda >= K && ldb >= K && ldh >= 2 * H && ldg >= H && 64 * ldb * 2 < (1LL << 32);      // the rest: launch_nt's refusals
}
int fk_mlp_up_fused_launch(const void* A, int64_t lda, const void* W13, int64_t ldb, void* H13, int64_t ldh, void* G, int64_t ldg, int64_t M, int64_t H,
                           void* stream) {
  MlpUpArgs a{(const bf16_t*)A, (const bf16_t*)W13, (bf16_t*)H13, (bf16_t*)G, lda, ldb, ldh, ldg, (int)M, (int)H};
  fk_launch_lds<mlp_up_fused_kernel>(dim3((unsigned)fk_cdiv(M, MU_TOK)), dim3(MU_NW * 64), MU_LDS, (hipStream_t)stream, a);
  FK_CHECK_LAUNCH("fk_gemm_nt_swiglu (token-on-the-lane kernel)");
  return FK_OK;
}

#ifdef MF_STAMP
extern "C" int fk_debug_mf_stamps(unsigned long long* out, int reset) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(mf_stamp_acc), sizeof(unsigned long long) * 16);
  if (reset) { unsigned long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(mf_stamp_acc), z, sizeof(z)); }
  return 0;
}
#endif

// whole 128-token tiles, and the dh13 rows addressable with 32-bit byte offsets from a per-chunk scalar base: the generated-stream kernel;
// everything else the kernel hipcc schedules (host only; fk_mlp_bwd_fused asks the same function)
extern "C" int fk_mlp_bwd_fused_route(int64_t M, int64_t lddh) {
  FK_CHECK_ARG(M > 0 && lddh > 0, "fk_mlp_bwd_fused_route: bad problem M=%lld lddh=%lld", (long long)M, (long long)lddh);
  return M % MF_TOK == 0 && M * lddh * 2 < (1LL << 32) ? FK_MLP_BWD_ASM : FK_MLP_BWD_HIPCC;
}

extern "C" int fk_mlp_bwd_fused(const void* dY, int64_t lddy, const void* W2T, int64_t ldw2t, const void* H13, int64_t ldh, const void* W13T,
                                int64_t ldw13t, void* dH13, int64_t lddh, void* dX, int64_t lddx, int64_t M, int64_t H, int64_t D, int dtype,
                                void* stream) {
  FK_CHECK_ARG(dtype == FK_BF16, "fk_mlp_bwd_fused: bf16 only (dtype %d)", dtype);
  FK_CHECK_ARG(D == MF_D, "fk_mlp_bwd_fused: model dimension %lld (built for %d)", (long long)D, MF_D);
  FK_CHECK_ARG(M > 0 && M < (1LL << 31) && H > 0 && H % 32 == 0 && H < (1 << 24), "fk_mlp_bwd_fused: bad shape M=%lld H=%lld", (long long)M, (long long)H);
  FK_CHECK_ARG(dY && W2T && H13 && W13T && dH13 && dX, "fk_mlp_bwd_fused: null pointer");
  FK_CHECK_ARG(lddy % 8 == 0 && ldw2t % 8 == 0 && ldh % 8 == 0 && ldw13t % 8 == 0 && lddh % 8 == 0 && lddx % 8 == 0 && lddy >= D && ldw2t >= D &&
                   ldh >= 2 * H && lddh >= 2 * H && ldw13t >= 2 * H && lddx >= D,
               "fk_mlp_bwd_fused: leading dimensions must be multiples of 8 elements and cover their rows");
  FK_CHECK_ARG(M * ldh * 2 < (1LL << 32) && (int64_t)D * ldw13t * 2 < (1LL << 32) && 32 * ldw2t * 2 < (1LL << 32),
               "fk_mlp_bwd_fused: the h13 block must be addressable with 32-bit byte offsets (M * ldh < 2^31 elements)");
  FK_CHECK_ARG((((uintptr_t)dY | (uintptr_t)W2T | (uintptr_t)H13 | (uintptr_t)W13T | (uintptr_t)dH13 | (uintptr_t)dX) & 15) == 0,
               "fk_mlp_bwd_fused: pointers must be 16-byte aligned");
  MlpBwdArgs a{(const bf16_t*)dY, (const bf16_t*)W2T, (const bf16_t*)H13, (const bf16_t*)W13T, (bf16_t*)dH13, (bf16_t*)dX,
               lddy, ldw2t, ldh, ldw13t, lddh, lddx, (int)M, (int)H};
  if (fk_mlp_bwd_fused_route(M, lddh) == FK_MLP_BWD_ASM)
    fk_launch_lds<mlp_bwd_fused_asm_kernel>(dim3((unsigned)(M / MF_TOK)), dim3(MF_NW * 64), MF_LDS, (hipStream_t)stream, a);
  else
    fk_launch_lds<mlp_bwd_fused_kernel>(dim3((unsigned)fk_cdiv(M, MF_TOK)), dim3(MF_NW * 64), MF_LDS, (hipStream_t)stream, a);
  FK_CHECK_LAUNCH("fk_mlp_bwd_fused");
  return FK_OK;
}
