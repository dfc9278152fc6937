// Internal building blocks of the GEMM launches (amx_gemm.hip): vector types, GemmArgs, the
// XCD-aware tile map, and the two f16x3 tile families (fp32 as two scaled fp16 limbs, three MFMA
// products) with the pieces their tile loops share.
#pragma once

#include "amx_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
// native vector (HIP's float4 is a wrapper struct: arrays of it were not promoted to registers)
typedef float f32x4 __attribute__((ext_vector_type(4)));

// EPI_MLPF: the feature layer of the MLP-feature MMD cost (MLPCost): EPI_RFF's staging, phi rows
// and fp64 column partials with phi = cos(tanh(z)) * scale in place of cos(z) * scale
enum { EPI_BIAS_ACT = 0, EPI_UNNORM = 1, EPI_RFF = 2, EPI_MLPF = 3 };
// the two feature epilogues (compile-time: the other kinds' kernels do not see them)
template <int EPI> constexpr bool epi_feature = EPI == EPI_RFF || EPI == EPI_MLPF;

struct GemmArgs {
  const float* A; long long strideA; int lda;
  const float* W; long long strideW; int ldw;
  const float* bias; long long strideBias;
  float* C; long long strideC; int ldc; int col_off;
  int rows, N, K;
  int act;                 // EPI_BIAS_ACT: AMX_ACT_*
  int n_valid;             // EPI_UNNORM: valid output columns; EPI_RFF / EPI_MLPF: valid rows
  const float* scale;      // EPI_UNNORM: sd_d
  const float* shift;      // EPI_UNNORM: mu_d
  float rff_scale;         // EPI_RFF / EPI_MLPF: sqrt(2/F)
  double* col_partials;    // EPI_RFF / EPI_MLPF: [rows/32][N] (AMX_RFF_PART_ROWS)
  const uint8_t* row_mask; // EPI_RFF / EPI_MLPF: nullable
  int tiles_m, tiles_n, groups;
  const uint16_t* W3;      // bf16x6 path: 3-limb weight image [g][N][K/16][3][16] (amx_split_bf16x3)
  long long strideW3;      //   elements between groups; a row is 3*K elements
  // f16x3 path (see the section below)
  const uint16_t* W2;      // 2-limb scaled weight image [g][N][K/16][2][16] (amx_split_f16x2)
  long long strideW2;
  const int* w_exp;        // [g][N] column exponents of W2 (strideWexp between groups)
  long long strideWexp;
  const int* row_exp;      // [g][slots][rows]: row exponents of A's column slices
  long long strideRexp;    //   between groups
  int rexp_slots;          //   slices of A read by this launch (exponent = max over them)
  int* row_exp_out;        // nullable: slot receiving the exponents of this launch's output rows
  int k_shared;            // leading K columns of A read from group 0's rows for every group
                           //   (the ensemble's x0 slice, assembled once; multiple of the tile's BK)
  int ksplit;              // partial-tile slots per tile in split_scratch (stream-K output layer)
  int streamk;             // > 0: stream-K over this many workgroups (16x16x32 tiles)
  float* split_scratch;    //   raw partial tiles [tile][slot][MB][NB][NT] f32x4 (amx_set_split_workspace)
  uint32_t* split_cnt;     //   arrivals per tile (zero between launches: the last arriver resets it)
  uint64_t* timer;         // amx_set_gemm_timer buffer (null: off)
  int timer_role;          //   1: first layer of a forward (block 0 stamps the start), 2: output layer
};

// Linear block id -> (group, tile_m, tile_n).  Workgroups are dispatched round-robin over
// the 8 XCDs, so block ids congruent mod 8 share an L2.  We hand each XCD a contiguous
// run of logical tiles (tile_n fastest: consecutive tiles reuse the same A row panel;
// then tile_m: they reuse the same weight panels of one ensemble member).  Bijective for
// any tile count (cdna_hip_programming.md T1).
__device__ inline int xcd_logical(int nwg, int orig) {
  const int xcd = orig & 7;
  const int q = nwg >> 3, r = nwg & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (orig >> 3);
}

__device__ inline void tile_coords(const GemmArgs& a, int logical, int& g, int& tm, int& tn) {
  tn = logical % a.tiles_n;
  const int rest = logical / a.tiles_n;
  tm = rest % a.tiles_m;
  g = rest / a.tiles_m;
}

__device__ inline void map_tile(const GemmArgs& a, int orig, int& g, int& tm, int& tn) {
  tile_coords(a, xcd_logical(a.tiles_m * a.tiles_n * a.groups, orig), g, tm, tn);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ==== f16x3: fp32 as two scaled fp16 limbs, three products ==================================
// x = 2^-s (x0 + x1) with x0 = RN_f16(2^s x) and x1 = RN_f16(2^s x - x0): 11 + 11 significant
// bits, |2^s x - x0 - x1| <= 2^-22 |2^s x| (or, below fp16's normal range, 2^-25 absolute
// against a row maximum scaled to [2^13, 2^14)).  a*b is then a0b0 + a0b1 + a1b0 on the f16
// matrix pipe with fp32 accumulation; the dropped a1b1 <= 2^-22 |ab|.  Over a K-long dot
// product these per-term errors add up like sqrt(K) * 2^-23 while the fp32 accumulation of
// the same sum rounds like K * 2^-24, so for K >= ~64 the result carries the same error as an
// fp32 GEMM (measured against fp64: tools/x6_accuracy.py) -- at 3 MFMA per 32x32x16 block
// instead of bf16x6's 6.
//
// The scales are powers of two, so they factor out of the contraction exactly:
//   * weights: per output column c, exponent E_c with max_k |W[c][k]| < 2^E_c, stored
//     scaled by 2^(14 - E_c) (amx_split_f16x2);
//   * activations: per row r, exponent E_r with max_k |A[r][k]| < 2^E_r, scaled by
//     2^(14 - E_r) while staged into LDS.  E_r = max over the row's column slices
//     (row_exp[g][slot][r]); the dense-concat rows are built slice by slice (x0, h0, h1, ...),
//     so the assembly writes slot 0 and each hidden layer's epilogue atomically max-es the
//     exponents of the slice it writes into its own slot (no slot is read and written by the
//     same launch: deterministic).
//   * epilogue: acc * 2^(E_r + E_c - 28) (one exact v_ldexp), then the fp32 bias etc. exactly
//     as the other paths.
// Exponents are clamped to [-100, 100] (zero rows, inf/NaN rows keep propagating as in fp32).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
constexpr int HSC = 14;  // scaled operands stay below 2^14 (fp16 max 65504)

__device__ __forceinline__ int exp_of_bits(uint32_t absbits) {
  // E with v < 2^E for v = |x| (bits of a non-negative float); clamped to [-100, 100]
  int e = (int)(absbits >> 23) - 126;
  e = e < -100 ? -100 : e;
  return e > 100 ? 100 : e;
}

// phi = cos(tanh(z)) * scale of MLPCost.get_rep (milo/milo/linear_cost.py:232-237: the net ends
// in Tanh, then torch.cos(.) * np.sqrt(2/F)), evaluated in fp64 and rounded to fp32 once.  phi of
// a default-initialised net sits within a few ulp of scale and w = mean phi_pi - mean phi_e is a
// difference of nearly equal means, so the budget is a fraction of an ulp of phi: rff_cos (3.5e-7
// absolute) and a 1-2 ulp fp32 tanh are both too coarse.  fp64 FMAs run at the fp32 rate on
// CDNA4's vector pipe and the epilogue is ~35 of them per element beside the K-loop's MFMAs.
//   tanh(z) = 1 - 2 / (e^2z + 1): e^2z = 2^n e^r with n = rint(2z / ln 2), |r| <= ln 2 / 2 (ln 2
//     in two parts, fma) and the degree-10 Taylor polynomial of e^r (r^11 / 11! < 3e-13); the
//     cancellation at small z is absolute (1e-16), which is what cos(t) needs (|dcos/dt| <= |t|);
//     2z is clamped to +-50 (tanh = +-1 to fp64 rounding), a NaN passes through both compares;
//   cos(t), |t| <= 1: the even Taylor polynomial through t^16 / 16! (next term 1.6e-16).
// Measured against long double over z in [-12, 12] and at the fp32 extremes: |error| <= 0.5 ulp
// of the fp32 result + 2e-16.  Host-callable, so the same code is checked on the CPU.
__host__ __device__ __forceinline__ float mlp_feature(float z, float scale) {
  double x = 2.0 * (double)z;
  x = x > 50.0 ? 50.0 : x;
  x = x < -50.0 ? -50.0 : x;
  const double n = __builtin_rint(x * 1.4426950408889634);
  double r = __builtin_fma(-n, 0.6931471803691238, x);  // ln 2: high part (low 21 bits clear: n * hi exact)
  r = __builtin_fma(-n, 1.9082149292705877e-10, r);
  double p = 2.7557319223985893e-07;                     // 1/10!
  p = __builtin_fma(p, r, 2.7557319223985888e-06);
  p = __builtin_fma(p, r, 2.4801587301587302e-05);
  p = __builtin_fma(p, r, 1.9841269841269841e-04);
  p = __builtin_fma(p, r, 1.3888888888888889e-03);
  p = __builtin_fma(p, r, 8.3333333333333332e-03);
  p = __builtin_fma(p, r, 4.1666666666666664e-02);
  p = __builtin_fma(p, r, 1.6666666666666666e-01);
  p = __builtin_fma(p, r, 0.5);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  const double d = __builtin_ldexp(p, (int)n) + 1.0;    // e^2z + 1 in [1, 5.2e21]
#if defined(__HIP_DEVICE_COMPILE__)
  double q = __builtin_amdgcn_rcp(d);                    // v_rcp_f64 + one Newton step
  q = __builtin_fma(__builtin_fma(-d, q, 1.0), q, q);
#else
  const double q = 1.0 / d;
#endif
  const double t = __builtin_fma(-2.0, q, 1.0);
  const double s = t * t;
  double c = 4.7794773323873853e-14;                     // 1/16!
  c = __builtin_fma(c, s, -1.1470745597729725e-11);      // -1/14!
  c = __builtin_fma(c, s, 2.08767569878681e-09);         // 1/12!
  c = __builtin_fma(c, s, -2.7557319223985888e-07);      // -1/10!
  c = __builtin_fma(c, s, 2.4801587301587302e-05);       // 1/8!
  c = __builtin_fma(c, s, -1.3888888888888889e-03);      // -1/6!
  c = __builtin_fma(c, s, 4.1666666666666664e-02);       // 1/4!
  c = __builtin_fma(c, s, -0.5);
  c = __builtin_fma(c, s, 1.0);
  return (float)(c * (double)scale);
}

// LDS of the RFF epilogue: a staged rows x (BN + 4) f32 tile
constexpr size_t rff_epi_lds(int rows, int bn) { return (size_t)rows * (bn + 4) * 4; }

// 32x32x16 form (v_mfma_f32_32x32x16_f16): WM x WN waves of TM x TN blocks of 32x32, NSUB 16-k
// granules per K-tile (BK = 16 NSUB), plain double buffer (one barrier per K-tile, the next
// tile's loads issued ahead of the MFMA block).  LDS row = NSUB x [limb0 16 | limb1 16] + 8 pad
// (20 dwords at NSUB 1, 36 at NSUB 2: the 16 rows of a ds_read_b128 lane group land on distinct
// 4-bank slots); the row exponents sit behind the two stage buffers.
// A-map (BK 32): the 16 lanes of a ds_write_b64 group stage rows r and r+2 (36-dword rows:
// 72 = 8 mod 32 banks apart, so their 2 x 8 dwords interleave) instead of r and r+1 (2-way
// bank conflict on every A limb store): 2% per layer (profiles/r01_h3_variants.txt)
template <int WM_, int WN_, int TM_, int TN_, int OCC_ = 2, int NSUB_ = 1>
struct TileH3 {
  static constexpr bool M16 = false;
  static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_, OCC = OCC_, NSUB = NSUB_, BK = 16 * NSUB_;
  static constexpr int LD = NSUB * 32 + 8;                     // f16 per LDS row
  static constexpr int NT = WM * WN * 64;
  static constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  static constexpr int STAGE = (BM + BN) * LD;                 // f16 of one stage (A + W)
  static constexpr size_t LDS = 2 * STAGE * sizeof(uint16_t) + BM * sizeof(int);
  static constexpr int SEXP = 2 * STAGE;                       // f16 offset of the row exponents
  static __device__ __forceinline__ int exp_word(int r) { return r; }  // dword of row r's exponent
  static constexpr int CPR = 4 * NSUB;                         // 16-B chunks per row and K-tile (A f32 and W)
  static constexpr int NA = BM * CPR, NW = BN * CPR;
  static constexpr int VA = (NA + NT - 1) / NT, VW = (NW + NT - 1) / NT;
  // rows of the RFF epilogue's staging pass (at three workgroups per CU: two 64-row passes)
  static constexpr int RFF_ROWS = OCC >= 3 ? BM / 2 : BM;
  static_assert(LDS <= 160 * 1024, "LDS");
};

// 16x16x32 form (v_mfma_f32_16x16x32_f16 on 16x16 blocks, BK 32; 4 fp32 accumulators per lane
// and block): the same cycles per FLOP as 32x32x16 at lower power per FLOP
// (MI355X_MICROARCH.md).  WM x WN waves of MB x NB blocks.  LDS rows of 40 dwords
// (conflict-free for its lane->k map and for the plain A staging map): 32 of limbs and 8 of
// padding, and the padding holds what must outlive the K loop -- the tile's row exponents (the
// 256 x 256 tile's stage buffers are all of the 160 KB), the epilogue's row maxima, the stream-K
// flag.
// Schedule (the guide's split write-after-barrier): barrier -> the first fragment reads of tile
// t -> per m-block, its MFMAs with the fragment reads of the next block pinned one MFMA group
// ahead (sched_barrier), then one piece of tile t+1's publish and of tile t+2's loads -- the LDS
// writes drain under the MFMAs, the loads get a whole K-tile.
// DEEPA: the A operand's loads run two K-tiles ahead of its publish instead of one (two register
// sets; the loop unrolled by two): the output layer's A panel is streamed from HBM once (N = 224
// columns per A row), so its K loop waits on load latency, not on the MFMAs
template <int WM_, int WN_, int MB_, int NB_, int OCC_ = 2, bool DEEPA_ = false>
struct TileH3M16 {
  static constexpr bool M16 = true, DEEPA = DEEPA_;
  static constexpr int WM = WM_, WN = WN_, MB = MB_, NB = NB_, OCC = OCC_, BK = 32;
  static constexpr int LD = 64 + 16;                           // f16 per LDS row
  static constexpr int NT = WM * WN * 64;
  static constexpr int WROWS = MB * 16, WCOLS = NB * 16;
  static constexpr int BM = WM * WROWS, BN = WN * WCOLS;
  static constexpr int STAGE = (BM + BN) * LD;                 // f16 of one stage (A + W)
  static constexpr size_t LDS = 2 * STAGE * sizeof(uint16_t);
  // Dword index (from the LDS base) of word i of buffer `stage`'s row padding: a stage row is 32
  // dwords of limbs + 8 of padding, which no staging write (a_dst / w_dst: f16 0..63 of the row)
  // and no fragment read (koff16 + 16 l + 8 <= 64) touches, so words kept there survive the K
  // loop.  Words 4i..4i+3 are contiguous and 16-B aligned (one ds_read_b128).
  static constexpr int PADW = (LD - 64) / 2, PAD_WORDS = (BM + BN) * PADW;
  static __device__ __forceinline__ int pad_word(int stage, int i) {
    return stage * (STAGE / 2) + (i / PADW) * (LD / 2) + 32 + i % PADW;
  }
  // the tile's combined row exponents: buffer 0's padding (BM words)
  static __device__ __forceinline__ int exp_word(int r) { return pad_word(0, r); }
  static_assert(PADW == 8 && BM <= PAD_WORDS, "row-exponent home");
  static constexpr int CPR = 8;                                // 16-B chunks per row and K-tile (A f32 and W)
  static constexpr int NA = BM * CPR, NW = BN * CPR;
  static constexpr int VA = (NA + NT - 1) / NT, VW = (NW + NT - 1) / NT;
  // rows of the RFF epilogue's staging pass: the whole tile when its [BM][BN + 4] floats fit
  // 80 KB, else the largest multiple of 32 rows that does (the 160 x 256 tile: 64 rows)
  static constexpr int RFF_ROWS =
      rff_epi_lds(BM, BN) <= 80 * 1024 ? BM : (int)((80 * 1024) / ((size_t)(BN + 4) * 4 * 32)) * 32;
  static_assert(LDS <= 160 * 1024, "LDS");
};

// 4 consecutive k of one row, pre-scaled -> two f16 limbs packed as 4 f16 each
__device__ __forceinline__ void split2(f32x4 x, u32x2& l0, u32x2& l1) {
  const f16x4 h0 = __builtin_convertvector(x, f16x4);
  const u32x2 hb = __builtin_bit_cast(u32x2, h0);
  // r1 = x - h0, exact: one mixed-precision fma per element (h0's f16 half widened inside
  // v_fma_mix_f32) instead of a widening convert and a subtract (hipcc folds an fmaf of a
  // widened half back into the convert + subtract, hence the asm)
  f32x4 r1;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r1[0]) : "v"(hb[0]), "v"(x[0]));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1[1]) : "v"(hb[0]), "v"(x[1]));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r1[2]) : "v"(hb[1]), "v"(x[2]));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1[3]) : "v"(hb[1]), "v"(x[3]));
  const f16x4 h1 = __builtin_convertvector(r1, f16x4);
  l0 = __builtin_bit_cast(u32x2, h0);
  l1 = __builtin_bit_cast(u32x2, h1);
}

// One reduce-scatter step of a max over the 32 lanes li: lanes with bit MASK set keep the upper
// HALF values, their partners the lower; each receives the other half (ds_swizzle bitmask
// mode: and 0x1f, xor MASK within 32-lane groups) and keeps the max.
template <int MASK, int HALF>
__device__ __forceinline__ void rs_step(uint32_t* v, int li) {
  const bool up = (li & MASK) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const uint32_t keep = up ? v[HALF + i] : v[i];
    const uint32_t send = up ? v[i] : v[HALF + i];
    const uint32_t recv = (uint32_t)__builtin_amdgcn_ds_swizzle((int)send, 0x1f | (MASK << 10));
    v[i] = keep > recv ? keep : recv;
  }
}

// amx_set_gemm_timer: the last workgroup of a forward's output layer adds (now - start) to the
// tick sum (stamps only in a buffer nothing else reads)
__device__ __forceinline__ void gemm_timer_end(const GemmArgs& a) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t nwg = gridDim.x;
    if (atomicAdd(reinterpret_cast<unsigned long long*>(a.timer + 1), 1ull) == nwg - 1) {
      const uint64_t now = __builtin_amdgcn_s_memrealtime();
      atomicAdd(reinterpret_cast<unsigned long long*>(a.timer + 2), (unsigned long long)(now - a.timer[0]));
      atomicAdd(reinterpret_cast<unsigned long long*>(a.timer + 3), 1ull);
      atomicExch(reinterpret_cast<unsigned long long*>(a.timer + 1), 0ull);
    }
  }
}

typedef __attribute__((address_space(1))) uint32_t gu32s;

// Stream-K combine (the output layer at lane counts whose 128 x 224 tiles are fewer than the
// CUs: the tiles' K-tiles are dealt out evenly over one workgroup per CU, so a tile's K range is
// covered by nseg <= 3 consecutive workgroups): every segment stores its raw (scaled)
// accumulators write-through (sc1, 16-B per lane) in its slot, drains, and adds to the tile's
// arrival counter (agent scope); the last arriver acquires, sums the segments in K order --
// P0 + P1 + ... whatever the arrival order, so the result is deterministic -- resets the
// counter and returns true to run the epilogue (cdna_hip_programming.md §5, in-launch split-K:
// one release and one acquire per tile).
template <class TL>
__device__ __forceinline__ bool split_combine(const GemmArgs& a, f32x4 (&acc)[TL::MB][TL::NB], int tile, int seg,
                                              int nseg, int* flag) {
  constexpr int MB = TL::MB, NB = TL::NB, NT = TL::NT;
  const int t = threadIdx.x;
  const long long per_slice = (long long)MB * NB * NT;  // f32x4 per slot
  f32x4* base = reinterpret_cast<f32x4*>(a.split_scratch) + (long long)tile * a.ksplit * per_slice;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7ffffff0, 0x00020000);
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NB; ++n)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[m][n]), rs,
                                             (int)(((seg * MB + m) * NB + n) * NT + t) * 16, 0, 16 /* sc1 */);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) {
    const uint32_t old = __hip_atomic_fetch_add((gu32s*)(a.split_cnt + tile), 1u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == (uint32_t)(nseg - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store((gu32s*)(a.split_cnt + tile), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    *flag = last;
  }
  __syncthreads();
  if (!*flag) return false;
  if constexpr (TL::NT <= 512 && MB * NB * TL::NT <= 2048) {
    // the small-row tiles (HS64 / HS32, 4 or 8 waves): the loads of four segments in flight
    // per round trip (each a write-through partial in memory, ~1-2 us away), then the sums in K
    // order -- v = P0, v += P1, ... exactly as below
    f32x4 v[MB][NB];
    for (int s0 = 0; s0 < nseg; s0 += 4) {
      f32x4 p[4][MB][NB];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int s = s0 + q;
        if (s < nseg && s != seg) {
#pragma unroll
          for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int n = 0; n < NB; ++n)
              p[q][m][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                         rs, (int)(((s * MB + m) * NB + n) * NT + t) * 16, 0, 16));
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int s = s0 + q;
        if (s < nseg) {
#pragma unroll
          for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int n = 0; n < NB; ++n) {
              const f32x4 x = s == seg ? acc[m][n] : p[q][m][n];
              v[m][n] = s == 0 ? x : v[m][n] + x;
            }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int n = 0; n < NB; ++n) acc[m][n] = v[m][n];
    return true;
  }
  // per block: v = P0, v += P1, ... (own segment from the accumulators) -- the segments' sum in
  // K order without a second copy of the accumulators (which spilled the 128-accumulator tiles).
  // (Round 4: reading this segment's slot back with the others so every segment's loads are in
  // flight together measured no faster at the N = 8 share, profiles/r04a_share_ab.txt.)
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const f32x4 mine = acc[m][n];
      f32x4 v = mine;
      for (int s = 0; s < nseg; ++s) {
        const f32x4 p = s == seg ? mine
                                 : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                 rs, (int)(((s * MB + m) * NB + n) * NT + t) * 16, 0, 16));
        v = s == 0 ? p : v + p;
      }
      acc[m][n] = v;
    }
  return true;
}

}  // namespace
