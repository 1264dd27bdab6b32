// Split-fp16 implicit-GEMM convolution for gfx950 (MI355X): fp32-class accuracy at the
// fp16 matrix-core rate.
//
// Every fp32 operand x is split as  x = hi + lo * 2^-11,  hi = fp16(x),  lo = fp16((x - hi) * 2^11)
// (relative representation error 2^-24, i.e. fp32-grade), and a product is formed from three
// fp16 MFMAs accumulating in fp32:
//      main += a_hi * b_hi
//      corr += a_hi * b_lo + a_lo * b_hi            (both carry the 2^11 scale)
//      out   = main + corr * 2^-11                   (a_lo*b_lo ~ 2^-22 relative is dropped)
// v_mfma_f32_32x32x16_f16 retires 16 k per 32 cycles against 2 k per 64 cycles for the exact
// v_mfma_f32_32x32x2_f32, so three of them are 16/3 = 5.3x the fp32 MFMA rate.  Activations keep 4 B per
// element in HBM -- fp32, split while the halo tile is staged into LDS, or already split by the producer's
// epilogue (ConvArgs::in_split / out_split) -- and weights are split once at load time.  Every MFMA convolution
// of the detector runs here in the split-fp16 modes: 3x3 at dilation 1, 2, 4 and the 1x1s.
//
// Kernels, one header each (this file is the host side: weight packs, knobs, the kernel table and the planner):
//   conv_f16x3_w4d.h   conv_mfma_f16x3_w4d_kernel -- the dual-tile 4-wave family: Cin >= 64, Cout % 128 == 0 (80 % of the time)
//   conv_f16x3_pc.h    conv_mfma_f16x3_pc_kernel  -- the fused first pair conv1_1 -> conv1_2, producer / consumer waves
//   conv_f16x3_k1.h    conv_mfma_f16x3_k1_kernel  -- the 1x1 layers with Cout % 256 == 0 as a plain GEMM over flat pixels
//   conv_f16x3_h3.h    conv_mfma_f16x3_heads3_kernel -- the three shared-weight dilated heads (dilation 1 / 2 / 4) in ONE launch
//   conv_f16x3_8w.h    conv_mfma_f16x3_kernel     -- 8 waves: what the others cannot take (Cout 64, other 1x1s, unaligned views)
//   conv_f16x3_types.h vector types, the hi / lo split, the MFMA wrapper, conv1_1's K-slot map
//   conv_lds_layout.h  (through conv_common.h) every kernel's LDS regions and total, and the tile geometry they are made of
// Common structure: tile 256 px (16x16) x BN couts; a STAGE is one kernel row (3 taps) of one channel chunk: its weight
// slabs are double-buffered in LDS and arrive by LDS DMA; the halo tile is staged once per chunk and reused by all 9 taps.
// 8-wave / first-pair LDS rows are [hi: 32 halfs][lo: 32 halfs][16 B pad] = 144 B (conflict-free ds_read_b128 over
// consecutive rows); the dual-tile family has its own geometry: 16-channel chunks, planar halo tiles, unscaled low parts.
// Epilogues: the 4-wave and first-pair kernels run the MFMA as D[cout][pixel] and store from registers
// (conv_common.h conv_epilogue_regs*, conv_epilogue_pool_only); the 8-wave kernel runs D[pixel][cout] and transposes the
// tile through LDS (conv_stage_tile / conv_flush_tile).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "conv_common.h"

#include "conv_f16x3_types.h"
#include "conv_f16x3_8w.h"
#include "conv_f16x3_w4d.h"
#include "conv_f16x3_pc.h"
#include "conv_f16x3_k1.h"
#include "conv_f16x3_h3.h"

namespace shf {

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
size_t split16_conv_weight_halfs(int Cout, int Cin, int k) { return (size_t)Cout * (Cin / 32) * k * k * 72; }

// host-side round-to-nearest-even fp32 -> bf16, returned as the fp16-typed bit pattern the packs store
static _Float16 host_bf16_as_half(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) u |= 0x00400000u;                 // NaN stays a NaN
  else u += 0x7fffu + ((u >> 16) & 1u);
  const uint16_t b = (uint16_t)(u >> 16);
  _Float16 h;
  memcpy(&h, &b, 2);
  return h;
}

// (Cout,Cin,3,3) fp32 -> [Cin/32][ky][kx][Cout][hi 32 | lo 32 | 8 pad] fp16 (144-B rows = the LDS image)
// bf: the bf16 mode's pack -- hi = bf16(w) bit patterns, lo = 0
void pack_conv_weights_split16(const float* w, int Cout, int Cin, int k, void* dst_, bool bf) {
  _Float16* dst = (_Float16*)dst_;
  const int taps = k * k;
  memset(dst_, 0, split16_conv_weight_halfs(Cout, Cin, k) * 2);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int t = 0; t < taps; ++t) {
        const float x = w[((size_t)co * Cin + ci) * taps + t];
        const _Float16 h = bf ? host_bf16_as_half(x) : (_Float16)x;
        const _Float16 l = bf ? (_Float16)0 : (_Float16)((x - (float)h) * f16x3::LO_SCALE);
        const size_t row = (((size_t)(ci / 32) * taps + t) * Cout + co) * 72;
        dst[row + (ci % 32)] = h;
        dst[row + 32 + (ci % 32)] = l;
      }
}

// The fused first pair's pack (conv_f16x3_pc.h): (Cout,Cin,3,3) fp32 -> [Cin/32][ky][kx][Cout][8 x 8 halfs] fp16, 128-byte rows
// WITHOUT padding; the eight 16-byte pieces of cout row r -- hi k 0-7, 8-15, 16-23, 24-31, then lo (x 2^11) the same -- sit at
// slot (piece + (r >> 1)) mod 8, so that the 16 lanes of a ds_read_b128 group (16 consecutive rows, one logical piece)
// cover all 16 bank groups.  The 6 KB of LDS this saves against the 144-byte rows pay for the halo rows' padding there.
size_t split16r_conv_weight_halfs(int Cout, int Cin, int k) { return (size_t)Cout * (Cin / 32) * k * k * 64; }
void pack_conv_weights_split16r(const float* w, int Cout, int Cin, int k, void* dst_, bool bf) {
  _Float16* dst = (_Float16*)dst_;
  const int taps = k * k;
  memset(dst_, 0, split16r_conv_weight_halfs(Cout, Cin, k) * 2);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int t = 0; t < taps; ++t) {
        const float x = w[((size_t)co * Cin + ci) * taps + t];
        const _Float16 h = bf ? host_bf16_as_half(x) : (_Float16)x;
        const _Float16 l = bf ? (_Float16)0 : (_Float16)((x - (float)h) * f16x3::LO_SCALE);
        const size_t row = (((size_t)(ci / 32) * taps + t) * Cout + co) * 64;
        const int kk = ci % 32, rot = (co >> 1) & 7;
        dst[row + (((kk >> 3) + rot) & 7) * 8 + (kk & 7)] = h;
        dst[row + ((4 + (kk >> 3) + rot) & 7) * 8 + (kk & 7)] = l;
      }
}

size_t split16h_conv_weight_halfs(int Cout, int Cin, int k) { return (size_t)Cout * (Cin / 16) * k * k * 32; }

// (Cout,Cin,3,3) fp32 -> [Cin/16][ky][kx][Cout][4 x 8 halfs] fp16: 64-B rows, NO padding (every byte of the pack is
// fetched by every block: padding is weight traffic) = the dual-tile kernel's LDS image.  The four 16-byte pieces of a row
// -- hi k 0-7, hi k 8-15, lo k 0-7, lo k 8-15 -- are rotated by (row / 4) mod 4 so that the 16 lanes of a ds_read_b128
// group (16 consecutive rows, one piece each) still fall on 16 different bank groups.
// lo is NOT scaled here: lo = fp16(w s - hi) with one power of two s per layer that lifts the weights to [8, 16) at the top,
// so that the low parts of all but the tiniest weights are normal fp16 numbers (the MFMA honours subnormals anyway:
// tools/mfma_denorm.hip) and the three products share one accumulator.  Returns 1 / s for the epilogue.
float pack_conv_weights_split16h(const float* w, int Cout, int Cin, int k, void* dst_, bool bf) {
  _Float16* dst = (_Float16*)dst_;
  const int taps = k * k;
  float amax = 0.f;
  for (size_t i = 0; i < (size_t)Cout * Cin * taps; ++i) amax = std::max(amax, std::fabs(w[i]));
  int e = 0;
  if (amax > 0.f) e = (int)std::floor(std::log2(8.0 / (double)amax));
  e = std::max(-14, std::min(14, e));
  if (bf) e = 0;   // bf16 has fp32's exponent range: nothing to lift
  const float s = std::ldexp(1.0f, e);
  memset(dst_, 0, split16h_conv_weight_halfs(Cout, Cin, k) * 2);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int t = 0; t < taps; ++t) {
        const float x = w[((size_t)co * Cin + ci) * taps + t] * s;
        const _Float16 h = bf ? host_bf16_as_half(x) : (_Float16)x;
        const _Float16 l = bf ? (_Float16)0 : (_Float16)(x - (float)h);
        const size_t row = (((size_t)(ci / 16) * taps + t) * Cout + co) * 32;
        const int kk = ci % 16, rot = ((co & 127) >> 2) & 3;
        dst[row + (((kk >> 3) + rot) & 3) * 8 + (kk & 7)] = h;
        dst[row + ((2 + (kk >> 3) + rot) & 3) * 8 + (kk & 7)] = l;
      }
  return 1.0f / s;
}


const ConvKnobs& conv_knobs() {
  static const ConvKnobs k = [] {
    auto env_int = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    ConvKnobs q;
    q.w4_mode = env_int("SHF_F16X3_W4", -1);
    q.w4_mt = env_int("SHF_F16X3_W4_MT", 0);
    q.w4d_ntile = env_int("SHF_F16X3_W4D_NTILE", 0);
    q.w4_slim = env_int("SHF_F16X3_W4_SLIM", 1);
    q.heads3 = env_int("SHF_F16X3_HEADS3", 1);
    q.pc_tab = env_int("SHF_F16X3_PC_TAB", 1);
    q.pc = env_int("SHF_F16X3_PC", 1) != 0;
    q.pc_persist = env_int("SHF_F16X3_PC_PERSIST", 1) != 0;
    q.split_act = env_int("SHF_F16X3_SPLIT_ACT", 1) != 0;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 4)
      cus = 256;
    // SHF_CONV_CUS >= 1: the planner cuts the work as for a device (or a partition) of that many CUs -- launches only,
    // never a result; the clamp above is for the device's own count
    const int plan_cus = env_int("SHF_CONV_CUS", 0);
    q.cus = plan_cus >= 1 ? plan_cus : cus;
    return q;
  }();
  return k;
}

namespace {
// 16-byte aligned channel views: what the vector epilogues (LDS-transposed and register) need
bool views_aligned(const ConvArgs* as, int n) {
  for (int i = 0; i < n; ++i) {
    const ConvArgs& q = as[i];
    if ((q.out.cstride % 4) || (q.out.coff % 4) || ((uintptr_t)q.out.p & 15)) return false;
    if (q.pool.p && ((q.pool.cstride % 4) || (q.pool.coff % 4) || ((uintptr_t)q.pool.p & 15))) return false;
  }
  return true;
}
// the dual-tile family addresses its input with 32-bit BYTE offsets from the member's base
bool inputs_under_4gib(const ConvArgs* as, int n) {
  for (int i = 0; i < n; ++i)
    if ((unsigned long long)as[i].in.B * as[i].in.H * as[i].in.W * as[i].in.cstride * 4ull >= (1ull << 32)) return false;
  return true;
}
// (Cin 64 -- conv2_1 -- joined in round 3: as two single-tile 8-row blocks per CU it beats the 8-wave kernel, 0.67 vs 0.81 ms)
bool uses_w4(int Cin) { return conv_knobs().w4_mode < 0 ? Cin >= 64 : conv_knobs().w4_mode != 0; }
}  // namespace

void pack_first_conv_frags(const float* w, void* dst_, bool bf) {
  _Float16* dst = (_Float16*)dst_;
  for (int n = 0; n < 2; ++n)
    for (int kk = 0; kk < 2; ++kk)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int i = lane & 31, kh = lane >> 5, k = first_conv_slot_tap(kk, kh, j);
          const float x = k >= 0 ? w[(size_t)(n * 32 + i) * 27 + k] : 0.f;
          const _Float16 h = bf ? host_bf16_as_half(x) : (_Float16)x;
          const _Float16 l = bf ? (_Float16)0 : (_Float16)((x - (float)h) * f16x3::LO_SCALE);
          dst[(((size_t)(n * 2 + kk) * 2 + 0) * 64 + lane) * 8 + j] = h;
          dst[(((size_t)(n * 2 + kk) * 2 + 1) * 64 + lane) * 8 + j] = l;
        }
}

bool conv_f16x3_eligible(int Cin, int Cout, int k, int pad, int dil) {
  const bool dil_ok = dil == 1 || dil == 2 || dil == 4;
  if (k == 1) return pad == 0 && Cin % 32 == 0 && Cout % 64 == 0;
  return k == 3 && dil_ok && pad == dil && Cin % 32 == 0 && Cout % 64 == 0;
}

// 3x3: Cout % 128 == 0 and the Cin the knob gives the family; 1x1 (the GEMM kernel: all 256 couts of a pixel in one
// block): Cout % 256 == 0, no fused pool.  What the family writes must be 16-byte aligned (register epilogues).
bool conv_f16x3_family_shape(int Cin, int Cout, int k, int pad, int dil, bool pool, bool aligned) {
  if (!aligned || !uses_w4(Cin) || !conv_f16x3_eligible(Cin, Cout, k, pad, dil)) return false;
  return k == 1 ? !pool && Cout % 256 == 0 : Cout % 128 == 0;
}

// 4-wave family: 16-row tiles (MT 4) or 8-row tiles (MT 2)?  A launch runs in ceil(blocks / CUs) rounds of one block
// per CU; an 8-row block costs ~0.56 of a 16-row one (half the MFMAs, the same weight traffic per stage and the same
// prologue / epilogue latencies).  SHF_F16X3_W4_MT = 2 / 4 forces the choice (experiments).
// Short K loops (Cin <= 128: 24 stages) are the exception: there a block's prologue (first ~50 KB of weights and halo)
// and epilogue (the output tile's store burst) are a third of its life, and the single-tile 8-row variant -- 80 640 B of
// LDS (two halo buffers of 15 488 B, 2 x 3 weight slabs of 8 192 B, 512 B of biases), 200 registers: TWO blocks per CU
// (161 280 of the 163 840 B), one's epilogue under the other's K loop -- wins although it moves four times the weight
// bytes per MFMA of a two-tile 16-row block.  Measured per layer on one box (tools/variant_layers.sh, us under
// rocprofv3): conv2_2 1212 vs 1278, conv3_1 625 vs 672, head_1 102 vs 109; from Cin 256 up it loses (conv3_2 1186 vs 1134,
// conv4_2 1196 vs 1072).
static bool w4_short_k(const ConvArgs* as) { return as[0].in.C <= 128; }
// The SLIM form of those single 8-row tiles (conv_mfma_f16x3_w4d_slim_kernel: one halo buffer, a ring of four tap slabs --
// 48 768 B, within W4_SLIM_LDS_MAX, at most 168 registers): THREE blocks per CU, so that a block's prologue and epilogue hide under two K loops.
// Same bits.  Per layer on one box, us under rocprofv3, two against three per CU: conv2_1 714 vs 694, conv2_2 1181 vs 1142,
// conv3_1 637 vs 629 (profiles/short_k_slim_ab.json): every short-K layer takes it.  SHF_F16X3_W4_SLIM = 0 keeps the
// two-per-CU form (A/B, identity tests).
static bool w4_slim(const ConvArgs* as) { return conv_knobs().w4_slim != 0 && w4_short_k(as) && as[0].in.C >= 64; }

static int w4_pick_mt(const ConvArgs* as, int n, int nct, int cus) {
  if (conv_knobs().w4_mt == 2 || conv_knobs().w4_mt == 4) return conv_knobs().w4_mt;
  if (w4_short_k(as)) return 2;
  long long t4 = 0, t2 = 0;
  for (int i = 0; i < n; ++i) {
    const long long tx = (as[i].in.W + f16x3::TW - 1) / f16x3::TW, B = as[i].in.B;
    t4 += B * tx * ((as[i].in.H + 15) / 16);
    t2 += B * tx * ((as[i].in.H + 7) / 8);
  }
  const double c4 = (double)((t4 * nct + cus - 1) / cus), c2 = 0.56 * (double)((t2 * nct + cus - 1) / cus);
  return c2 < c4 ? 2 : 4;
}

// Every kernel instantiation of the split-fp16 modes, each with the profiler class its launches are booked under.  Columns:
// NP = 3, 2, 1 fp16 products, then bf16 (one product on bf16 operands); [IN_SPLIT x NP] = the fp32-input forms, the split-input
// forms, then bf16 (fp32 activations: no split input).
// What each column computes, operand by operand, and which cells the bit-exact tests (tests/test_gpu_conv_modes.py) reach
// and cannot reach: DESIGN.md, "Operand model of every mode, held bit for bit".
// An entry's LDS size is its layout's (conv_lds_layout.h), named by the same macro arguments as the kernel; conv_lds<>
// refuses at compile time a layout beyond the 160 KiB conv_set_lds_attributes asks for.
#define SHF_8W1(PC, BN, DIL, KS, FUSE1, ...) \
  {(const void*)conv_mfma_f16x3_kernel<BN, FUSE1, DIL, KS, __VA_ARGS__>, PC, conv_lds<W8Lds<BN, DIL, KS, FUSE1>>()}
#define SHF_8W(PC, BN, DIL, KS) \
  {SHF_8W1(PC, BN, DIL, KS, false, 3), SHF_8W1(PC, BN, DIL, KS, false, 2), SHF_8W1(PC, BN, DIL, KS, false, 1), SHF_8W1(PC, BN, DIL, KS, false, 1, true)}
#define SHF_PC1(PC, NP, BF, PERSIST) {(const void*)conv_mfma_f16x3_pc_kernel<NP, BF, PERSIST>, PC, conv_lds<PcLds>()}
#define SHF_PC(PC, PERSIST) {SHF_PC1(PC, 3, false, PERSIST), SHF_PC1(PC, 2, false, PERSIST), SHF_PC1(PC, 1, false, PERSIST), SHF_PC1(PC, 1, true, PERSIST)}
#define SHF_W4D1(PC, SPLIT, MT, NT, NP, BF, DIL) \
  {(const void*)conv_mfma_f16x3_w4d_kernel<SPLIT, MT, NT, NP, BF, DIL>, PC, conv_lds<W4dLds<MT, NT, DIL, false>>()}
#define SHF_W4D(PC0, PC1, MT, NT, DIL)                                                                                     \
  {SHF_W4D1(PC0, false, MT, NT, 3, false, DIL), SHF_W4D1(PC0, false, MT, NT, 2, false, DIL), SHF_W4D1(PC0, false, MT, NT, 1, false, DIL), \
   SHF_W4D1(PC1, true, MT, NT, 3, false, DIL), SHF_W4D1(PC1, true, MT, NT, 2, false, DIL), SHF_W4D1(PC1, true, MT, NT, 1, false, DIL),    \
   SHF_W4D1(PC0, false, MT, NT, 1, true, DIL)}
#define SHF_W4S1(PC, ...) {(const void*)conv_mfma_f16x3_w4d_slim_kernel<__VA_ARGS__>, PC, conv_lds<W4dLds<2, 1, 1, true>>()}
#define SHF_W4S(PC0, PC1)                                                                                                  \
  {SHF_W4S1(PC0, false, 3), SHF_W4S1(PC0, false, 2), SHF_W4S1(PC0, false, 1), SHF_W4S1(PC1, true, 3), SHF_W4S1(PC1, true, 2),  \
   SHF_W4S1(PC1, true, 1), SHF_W4S1(PC0, false, 1, true)}
#define SHF_2NP3(PC, K, L)                                                                                                 \
  {{(const void*)K<false, 3>, PC, conv_lds<L>()}, {(const void*)K<false, 2>, PC, conv_lds<L>()}, {(const void*)K<false, 1>, PC, conv_lds<L>()}, \
   {(const void*)K<true, 3>, PC, conv_lds<L>()}, {(const void*)K<true, 2>, PC, conv_lds<L>()}, {(const void*)K<true, 1>, PC, conv_lds<L>()}}
struct F16x3Kernels {
  ConvKernel w8_128[2][4];   // conv_mfma_f16x3_kernel at BN 128: [3x3 DIL 1, 1x1][NP] (its dilated forms would need 168 / 194 KB
                             // of LDS: dilated layers with Cout % 128 == 0 take BN 64 here, or the family's DIL form)
  ConvKernel w8_64[4][4];    // ... at BN 64: [DIL 1, 2, 4 (3x3), then 1x1][NP]
  ConvKernel w8_fuse1;       // ... conv1_1 computed in the halo staging
  ConvKernel pc[2][4];       // conv_mfma_f16x3_pc_kernel: [PERSIST][NP]
  ConvKernel w4d[2][2][7];   // conv_mfma_f16x3_w4d_kernel, DIL 1: [MT 4, 2][NTILE 2, 1][IN_SPLIT x NP]
  ConvKernel w4d_dil[2][7];  // ... single 16-row tiles at DIL 2, 4: [DIL][IN_SPLIT x NP]
  ConvKernel w4d_slim[7];    // ... the SLIM form of the single 8-row tiles, three blocks per CU: [IN_SPLIT x NP]
  ConvKernel k1[6];          // conv_mfma_f16x3_k1_kernel: [IN_SPLIT x NP]
  ConvKernel h3[6];          // conv_mfma_f16x3_heads3_kernel: [IN_SPLIT x NP]
};
#define SHF_W4D_PC(SPLIT, MT, NT) (PC_CONV_F16X3_W4D_0 + 4 * SPLIT + (MT == 2 ? 2 : 0) + (NT == 1 ? 1 : 0))
static const F16x3Kernels kK = {
    {SHF_8W(PC_CONV_F16X3_128, 128, 1, 3), SHF_8W(PC_CONV_F16X3_128_K1, 128, 1, 1)},
    {SHF_8W(PC_CONV_F16X3_64, 64, 1, 3), SHF_8W(PC_CONV_F16X3_64_D2, 64, 2, 3), SHF_8W(PC_CONV_F16X3_64_D4, 64, 4, 3),
     SHF_8W(PC_CONV_F16X3_64_K1, 64, 1, 1)},
    SHF_8W1(PC_CONV_F16X3_64_FUSE1, 64, 1, 3, true, 3),
    {SHF_PC(PC_CONV_F16X3_PC, false), SHF_PC(PC_CONV_F16X3_PCP, true)},
    {{SHF_W4D(SHF_W4D_PC(0, 4, 2), SHF_W4D_PC(1, 4, 2), 4, 2, 1), SHF_W4D(SHF_W4D_PC(0, 4, 1), SHF_W4D_PC(1, 4, 1), 4, 1, 1)},
     {SHF_W4D(SHF_W4D_PC(0, 2, 2), SHF_W4D_PC(1, 2, 2), 2, 2, 1), SHF_W4D(SHF_W4D_PC(0, 2, 1), SHF_W4D_PC(1, 2, 1), 2, 1, 1)}},
    {SHF_W4D(PC_CONV_F16X3_W4D_D2, PC_CONV_F16X3_W4D_D2, 4, 1, 2), SHF_W4D(PC_CONV_F16X3_W4D_D4, PC_CONV_F16X3_W4D_D4, 4, 1, 4)},
    SHF_W4S(SHF_W4D_PC(0, 2, 1), SHF_W4D_PC(1, 2, 1)),
    SHF_2NP3(PC_CONV_F16X3_K1G, conv_mfma_f16x3_k1_kernel, K1Lds),
    SHF_2NP3(PC_CONV_F16X3_H3, conv_mfma_f16x3_heads3_kernel, H3Lds)};
#undef SHF_W4D_PC
#undef SHF_2NP3
#undef SHF_W4S
#undef SHF_W4S1
#undef SHF_W4D
#undef SHF_W4D1
#undef SHF_PC
#undef SHF_PC1
#undef SHF_8W
#undef SHF_8W1
static_assert(sizeof(F16x3Kernels) % sizeof(ConvKernel) == 0, "the attribute set-up walks the table as one array");

int conv_f16x3_init_attributes() {
  (void)conv_knobs();
  return conv_set_lds_attributes((const ConvKernel*)&kK, (int)(sizeof(kK) / sizeof(ConvKernel)));
}

static int np_col(const ConvArgs& a) { return a.bf16 ? 3 : a.nprod >= 3 ? 0 : a.nprod == 2 ? 1 : 2; }   // [NP]
static int split_col(const ConvArgs& a) { return a.bf16 ? 6 : 3 * (a.in_split ? 1 : 0) + np_col(a); }  // [IN_SPLIT x NP]

#ifdef SHF_CONV_TIMING
static unsigned long long* timing_buffer() {
  static unsigned long long* dbg_dev = nullptr;
  if (!dbg_dev) hipMalloc((void**)&dbg_dev, 16 * 5 * 8);
  hipMemset(dbg_dev, 0, 16 * 5 * 8);
  return dbg_dev;
}
// the family's per-block phase sums (conv_f16x3_w4d.h): wave 0 of every block of the layer's launch(es)
static void w4d_timing_report(const ConvPlan& pl, hipStream_t s) {
  unsigned long long h[4];
  hipStreamSynchronize(s);
  hipMemcpy(h, pl.k.dbg, sizeof(h), hipMemcpyDeviceToHost);
  const ConvK& p = pl.k;
  if (h[3])
    fprintf(stderr, "[w4d timing] Cin %d Cout %d rows %d: %llu blocks, per block cycles: prologue %.0f, K loop %.0f (%d stages: %.0f each), epilogue %.0f\n",
            p.Cin, p.Cout, pl.rows, h[3], (double)h[0] / h[3], (double)h[1] / h[3], p.Cin / 16 * 3, (double)h[1] / h[3] / (p.Cin / 16 * 3),
            (double)h[2] / h[3]);
}
static void f16x3_timing_report(const ConvPlan& pl, hipStream_t s) {
  unsigned long long h[80];
  hipStreamSynchronize(s);
  hipMemcpy(h, pl.k.dbg, sizeof(h), hipMemcpyDeviceToHost);
  for (int w = 0; w < 16; w += 3)
    if (h[w * 5 + 4])
      fprintf(stderr, "[f16x3 timing] blk%d wave%d stages %llu: per-stage cycles barrier %.0f issue %.0f compute %.0f tail %.0f\n",
              w / 8 ? 100 : 0, w % 8, h[w * 5 + 4], (double)h[w * 5] / h[w * 5 + 4], (double)h[w * 5 + 1] / h[w * 5 + 4],
              (double)h[w * 5 + 2] / h[w * 5 + 4], (double)h[w * 5 + 3] / h[w * 5 + 4]);
}
#endif

// The split-fp16 modes: the fused first pair (producer / consumer kernel, or the 8-wave kernel's FUSE1 form), the dual-tile
// family (1x1: the GEMM kernel; dilated heads: single 16-row tiles; dilation 1: two-tile / single-tile blocks, 16 or 8 rows),
// and the 8-wave kernel for what the others cannot take (Cout 64, other 1x1s, unaligned views, inputs of 4 GiB or more).
// `plan_cus` >= 1 (the plan probes only): plan for that many CUs instead of conv_knobs().cus.
ConvPlan plan_conv_f16x3(const ConvArgs* as, int n, int plan_cus) {
  using namespace f16x3;
  const ConvKnobs& kn = conv_knobs();
  const int cus = plan_cus >= 1 ? plan_cus : kn.cus;
  const ConvArgs& a = as[0];
  ConvPlan pl;
  if (a.img && (a.in.C != 64 || !a.w1t)) { pl.err = "conv f16x3: fused first layer needs 64 channels + transposed weights"; return pl; }
  const bool vec_ok = views_aligned(as, n);   // (unaligned channel views: the 8-wave kernel's scalar stores)
  const bool family = a.wsplit16h && !a.img && !(a.k == 1 && a.bf16) && inputs_under_4gib(as, n) &&
                      conv_f16x3_family_shape(a.in.C, a.out.C, a.k, a.pad, a.dil, a.pool.p != nullptr, vec_ok);
  const bool dual = family && a.k == 3 && a.dil == 1;
  const int BN = family ? (a.k == 1 ? 256 : 128) : (a.img || a.out.C % 128 || (a.k == 3 && a.dil != 1)) ? 64 : 128;
  const int nct = a.out.C / BN;
  const int mt = dual ? w4_pick_mt(as, n, nct, cus) : 4;
  const long long tiles = conv_fill(pl, as, n, nct, family && a.k == 1 ? 0 : 4 * mt, family && a.k == 1 ? 256 : TW);
  if (tiles < 0) return pl;
  ConvK& p = pl.k;
  p.wp = (const float*)a.wsplit16;
  if (family) {
    p.wph = a.wsplit16h;
    p.wscale_inv = a.wscale_inv;
  }
  p.w1t = a.w1t; p.w1f = a.w1f; p.b1 = a.b1;
  if (a.k == 1) p.dil = 1;
  if (vec_ok) p.flags |= CONV_VEC_EPI;
  if (a.out_split || a.pool_split) {
    if (!vec_ok) { pl.err = "conv f16x3: split-format output needs the aligned epilogue"; return pl; }
    p.flags |= (a.out_split ? CONV_MAIN_SPLIT : 0) | (a.pool_split ? CONV_POOL_SPLIT : 0);
  }
  auto add = [&](const ConvKernel& kern, long long grid, int block, long long tile_base, long long ntile_blocks, double share) {
    pl.l[pl.nl++] = {&kern, dim3((unsigned)grid), dim3(block), kern.lds, (int)tile_base, (int)ntile_blocks, share};
  };
#ifdef SHF_CONV_TIMING
  if (!(family && a.k == 1)) {
    p.dbg = timing_buffer();
    pl.timing_report = dual ? w4d_timing_report : f16x3_timing_report;
    pl.rows = 4 * mt;
  }
#endif
  if (family && a.k == 1) {   // blocks of 256 pixels of each member's flat pixel list x 256 couts
    add(kK.k1[split_col(a)], tiles * nct, 256, 0, 0, 1.0);
    return pl;
  }
  if (a.img && kn.pc && vec_ok && a.out.C == 64 && a.w1f && a.wsplit16r) {
    p.wp = (const float*)a.wsplit16r;   // its own pack: 128-byte rotated rows (pack_conv_weights_split16r)
    if (!kn.pc_persist) {
      add(kK.pc[0][np_col(a)], tiles, 512, 0, 0, 1.0);
      return pl;
    }
    // one block per CU walks the tiles (tile = block, block + grid, ...)
    const long long grid = std::min<long long>(tiles, cus);
    // the per-block tile table: fits (PC_TABN = 300 tiles per block) and packs (image < 256, tile row / column < 1024)?
    bool ok = kn.pc_tab != 0 && (tiles + grid - 1) / grid <= PcLds::PC_TABN;
    for (int i = 0; i < n; ++i)
      ok = ok && as[i].in.B <= 255 && p.m[i].tiles_x <= 1023 && p.m[i].tiles_per_img / std::max(1, p.m[i].tiles_x) <= 1023;
    p.pc_tab = ok ? 1 : 0;
    add(kK.pc[1][np_col(a)], grid, 512, 0, tiles, 1.0);
    return pl;
  }
  if (family && a.dil > 1) {
    // the dilated heads on the family's DIL form: single 16-row tiles (halo tiles of (16 + 2 DIL)^2 pixels, two buffer sets)
    add(kK.w4d_dil[a.dil == 4][split_col(a)], tiles * nct, 256, 0, tiles * nct, 1.0);
    return pl;
  }
  if (dual) {
    // dual-tile family (conv_mfma_f16x3_w4d_kernel<.., MT, NTILE, ..>): every variant forms an output with the same
    // operations in the same order, so the choice below -- two tiles per block where that fills whole rounds of one
    // block per CU, single tiles for the rest -- never changes a result.
    const long long per_round = cus / nct > 0 ? cus / nct : 1;   // pixel tiles (single) or pairs (dual) per round
    const long long pairs = (tiles + 1) / 2;
    const double c1 = mt == 4 ? 1.0 : 0.56, c2 = mt == 4 ? 1.82 : 1.02;   // block cost: one / two tiles (w4_pick_mt's unit)
    const long long full2 = pairs / per_round;                  // whole rounds of dual blocks
    const long long rest = std::max(0LL, tiles - 2 * full2 * per_round);
    const double cost_all1 = c1 * (double)((tiles + per_round - 1) / per_round);
    const double cost_all2 = c2 * (double)((pairs + per_round - 1) / per_round);
    const double cost_hyb = c2 * (double)full2 + c1 * (double)((rest + per_round - 1) / per_round);
    long long n2 = 0;                                           // pixel tiles covered by the dual launch
    if (cost_all2 <= cost_all1 && cost_all2 <= cost_hyb) n2 = tiles;
    else if (cost_hyb < cost_all1) n2 = 2 * full2 * per_round;
    if (w4_short_k(as) && kn.w4_mt == 0) n2 = 0;               // two single-tile blocks per CU (w4_pick_mt)
    if (kn.w4d_ntile == 1) n2 = 0;
    if (kn.w4d_ntile == 2) n2 = tiles;
    const auto& fam = kK.w4d[mt == 2];
    // the slim single-tile form (a third of a CU's LDS at the most: W4_SLIM_LDS_MAX)
    const bool slim = mt == 2 && n2 == 0 && w4_slim(as);
    if (n2 > 0) add(fam[0][split_col(a)], ((n2 + 1) / 2) * nct, 256, 0, n2 * nct, (double)n2 / (double)tiles);
    if (n2 < tiles)
      add(slim ? kK.w4d_slim[split_col(a)] : fam[1][split_col(a)], (tiles - n2) * nct, 256, n2, tiles * nct,
          (double)(tiles - n2) / (double)tiles);
    return pl;
  }
  if (a.in_split) {
    pl.err = "conv f16x3: split-format input reached a kernel other than the 4-wave family (unaligned views, or an input of 4 GiB or more)";
    return pl;
  }
  if (a.bf16 && a.img) { pl.err = "conv f16x3: bf16 mode runs the first pair on the producer/consumer kernel only"; return pl; }
  // 8-wave kernel; BN is 128 only at dilation 1 and for 1x1 layers (above)
  const int dcol = a.k == 1 ? 3 : a.dil / 2;   // [DIL 1, 2, 4, then 1x1]
  add(a.img ? kK.w8_fuse1 : BN == 128 ? kK.w8_128[a.k == 1][np_col(a)] : kK.w8_64[dcol][np_col(a)], tiles * nct, 512, 0, 0, 1.0);
  return pl;
}

// diagnostics (shf_debug_conv_plan): the launches the planner gives a 3x3 / dilation-1 layer of the split-fp16 mode on one
// (1, H, W) unit.  Nothing is launched and no device memory is touched: the views only have to look aligned.
int conv_f16x3_plan_probe(int Cin, int Cout, int H, int W, int in_split, int pooled, long long* lds, long long* grid, int* slim) {
  alignas(16) static float dummy[4];
  ConvArgs a;
  a.in = View{dummy, 1, H, W, Cin, Cin, 0};
  a.out = View{dummy, 1, H, W, Cout, Cout, 0};
  if (pooled) a.pool = View{dummy, 1, (H + 1) / 2, (W + 1) / 2, Cout, Cout, 0};
  a.wsplit16 = dummy;
  a.wsplit16h = dummy;
  a.in_split = in_split ? 1 : 0;
  const ConvPlan pl = plan_conv_f16x3(&a, 1);
  if (pl.nl == 0) { set_error(pl.err.empty() ? "conv f16x3: no plan" : pl.err); return -1; }
  for (int i = 0; i < pl.nl; ++i) {
    lds[i] = (long long)pl.l[i].lds;
    grid[i] = (long long)pl.l[i].grid.x;
    slim[i] = pl.l[i].kern >= kK.w4d_slim && pl.l[i].kern < kK.w4d_slim + 7 ? 1 : 0;
  }
  return pl.nl;
}

// diagnostics (shf_debug_conv_plan_group): the launches of a grouped pass over n (b[i], h[i], w[i]) units (b null: 1) -- the dual-tile
// family's cover, or with first_pair the plan of conv1_2 fused with conv1_1 (64 -> 64) -- planned for `cus` CUs (0: the
// knob's or the device's).  out[8 * launch ..]: grid, LDS bytes, tile rows, tiles per block, tile_base, ntile_blocks, slim,
// persistent; *pc_tab: ConvK::pc_tab.  Nothing is launched and no device memory is touched.
int conv_f16x3_plan_probe_group(int n, const int* B, const int* H, const int* W, int Cin, int Cout, int in_split, int pooled, int first_pair,
                                int cus, long long* out, int* pc_tab) {
  alignas(16) static float dummy[4];
  if (n < 1 || n > MAX_GROUP) { set_error("conv plan probe: 1..16 members"); return -1; }
  ConvArgs as[MAX_GROUP];
  for (int i = 0; i < n; ++i) {
    ConvArgs& a = as[i];
    const int b = B ? B[i] : 1;
    a.in = View{dummy, b, H[i], W[i], Cin, Cin, 0};
    a.out = View{dummy, b, H[i], W[i], Cout, Cout, 0};
    if (pooled) a.pool = View{dummy, b, (H[i] + 1) / 2, (W[i] + 1) / 2, Cout, Cout, 0};
    a.wsplit16 = dummy;
    a.in_split = in_split ? 1 : 0;
    if (first_pair) {
      a.img = dummy; a.w1t = dummy; a.w1f = dummy; a.b1 = dummy; a.wsplit16r = dummy;
    } else {
      a.wsplit16h = dummy;
    }
  }
  const ConvPlan pl = plan_conv_f16x3(as, n, cus);
  if (pl.nl == 0) { set_error(pl.err.empty() ? "conv f16x3: no plan" : pl.err); return -1; }
  for (int i = 0; i < pl.nl; ++i) {
    const ConvLaunch& L = pl.l[i];
    const ConvKernel* k = L.kern;
    const bool slim = k >= kK.w4d_slim && k < kK.w4d_slim + 7, pc = k >= &kK.pc[0][0] && k < &kK.pc[0][0] + 8;
    const bool w4 = k >= &kK.w4d[0][0][0] && k < &kK.w4d[0][0][0] + 28;
    int rows = 16, ntile = 1;   // (the first pair and the 8-wave kernel: 16-row tiles, one at a time)
    if (slim) rows = 8;
    if (w4) {
      const int idx = (int)(k - &kK.w4d[0][0][0]) / 7;   // [MT 4, 2][NTILE 2, 1]
      rows = idx / 2 ? 8 : 16;
      ntile = idx % 2 ? 1 : 2;
    }
    long long* o = out + 8 * i;
    o[0] = (long long)L.grid.x; o[1] = (long long)L.lds; o[2] = rows; o[3] = ntile; o[4] = L.tile_base; o[5] = L.ntile_blocks;
    o[6] = slim ? 1 : 0;
    o[7] = pc && k >= &kK.pc[1][0] ? 1 : 0;
  }
  *pc_tab = pl.k.pc_tab;
  return pl.nl;
}

// The three shared-weight dilated heads as ONE launch (conv_f16x3_h3.h): a1 / a2 / a4 = the dilation-1 / 2 / 4 layers'
// arguments, member by member.  They must read the same input with the same weights and differ in dilation and output only.
static bool heads3_qualifies(const ConvArgs* a1, const ConvArgs* a2, const ConvArgs* a4, int n) {
  if (!conv_knobs().heads3 || n < 1 || n > MAX_GROUP) return false;
  const ConvArgs& a = a1[0];
  if (!a.wsplit16h || a.bf16 || a.img || a.k != 3 || a.dil != 1 || a.out.C != 128 || a.in.C % 16 || !uses_w4(a.in.C)) return false;
  for (int i = 0; i < n; ++i) {
    const ConvArgs* q[3] = {&a1[i], &a2[i], &a4[i]};
    if (q[1]->dil != 2 || q[2]->dil != 4) return false;
    for (int d = 0; d < 3; ++d) {
      const ConvArgs& b = *q[d];
      if (b.k != 3 || b.pad != b.dil || b.wsplit16h != a.wsplit16h || b.bias != a.bias || b.nprod != a.nprod || b.bf16 || b.pool.p ||
          b.relu != a.relu || b.in_split != a.in_split || b.out_split != a.out_split || b.out.C != 128 || b.out.cstride != a.out.cstride ||
          b.in.p != q[0]->in.p || b.in.coff != q[0]->in.coff || b.in.cstride != a.in.cstride || b.in.C != a.in.C ||
          b.in.B != q[0]->in.B || b.in.H != q[0]->in.H || b.in.W != q[0]->in.W || b.range_flag != a.range_flag)
        return false;
    }
    if (!views_aligned(q[0], 1) || !views_aligned(q[1], 1) || !views_aligned(q[2], 1) || !inputs_under_4gib(q[0], 1)) return false;
  }
  return true;
}

ConvPlan plan_conv_heads3(const ConvArgs* a1, const ConvArgs* a2, const ConvArgs* a4, int n) {
  ConvPlan pl;
  if (!heads3_qualifies(a1, a2, a4, n)) return pl;
  const long long tiles = conv_fill(pl, a1, n, 1, 8, 16);
  if (tiles < 0) return pl;
  const ConvArgs& a = a1[0];
  ConvK& p = pl.k;
  p.wp = (const float*)a.wsplit16;
  p.wph = a.wsplit16h;
  p.wscale_inv = a.wscale_inv;
  p.flags |= CONV_VEC_EPI | (a.out_split ? CONV_MAIN_SPLIT : 0);
  for (int i = 0; i < n; ++i) {
    ConvMember& m = p.m[i];
    m.out2 = a2[i].out.p + a2[i].out.coff;
    m.out3 = a4[i].out.p + a4[i].out.coff;
    m.out2_amax = a2[i].out_amax;
    m.out3_amax = a4[i].out_amax;
  }
  const ConvKernel& kern = kK.h3[split_col(a)];
  pl.l[pl.nl++] = {&kern, dim3((unsigned)tiles), dim3(256), kern.lds, 0, (int)tiles, 1.0};
  return pl;
}

}  // namespace shf
