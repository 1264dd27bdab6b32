// The dynamic LDS of every MFMA convolution kernel: one layout per kernel, templated on exactly the parameters that decide
// it.  A layout's members are the offsets of the regions the kernel addresses and `bytes`, the total; the kernel takes its
// pointers from them (smem + L::region) and the kernel tables (conv.hip, conv_f16x3.hip) take the launch's size from them
// (ConvKernel::lds), so a region added here reaches both or neither.  The tile-geometry constants the layouts are made
// of live here too, once.  Plain constexpr for host and device code; the totals are pinned at the end of the file.
#pragma once
#include <cstddef>

namespace shf {

constexpr size_t CONV_LDS_OPT_IN = 160 * 1024;   // what conv_set_lds_attributes asks for: all of a CU's LDS

// a layout's size for a kernel-table entry; an instantiation that cannot be launched does not compile
template <class L>
constexpr size_t conv_lds() {
  static_assert(L::bytes <= CONV_LDS_OPT_IN, "the kernel's LDS layout does not fit a compute unit");
  return L::bytes;
}

// ---- exact fp32 kernel (conv.hip: conv_mfma_f32_kernel<KS, DIL, BN, TH, 16>).  Its smem is float[]: offsets in FLOATS.
constexpr int LDK = 36;  // LDS row pitch in floats (32 + 4 pad: conflict-free ds_read_b128)
template <int KS, int DIL, int BN, int TH>
struct F32Lds {
  static constexpr int PAD = KS == 3 ? DIL : 0, HP = (TH + 2 * PAD) * (16 + 2 * PAD);
  static constexpr int As = 0;               // [HP][LDK]
  static constexpr int Bs = HP * LDK;        // [2][BN][LDK]
  static constexpr size_t bytes = (size_t)(Bs + 2 * BN * LDK) * sizeof(float);
};

// ---- split-fp16 kernels (conv_f16x3.hip): byte offsets
namespace f16x3 {
constexpr int KC = 32;      // input channels per chunk
constexpr int ROWB = 144;   // bytes per LDS row (pixel or cout)
constexpr int TH = 16, TW = 16, HTW = TW + 2, HTH = TH + 2, HP = HTH * HTW;
}  // namespace f16x3

// the LDS-transposed epilogue tile Cs[256 pixels][BN + CS_PAD] floats (conv_common.h: conv_stage_tile / conv_flush_tile)
constexpr int CS_PAD = 16;  // 2 x (BN + CS_PAD) words = 32 (mod 64 banks): the two half-waves of a staging ds_write_b32 (pixels x, x+2) never share a bank

// 8-wave kernel (conv_f16x3_8w.h: conv_mfma_f16x3_kernel<BN, FUSE1, DIL, KS, ..>).  The output tile is transposed
// through the K loop's buffers once they are dead (the 1x1 forms' are smaller than the tile); the FUSE1 extras sit behind
// the weight buffers and are counted behind whichever of the two is larger.
template <int BN, int DIL, int KS, bool FUSE1>
struct W8Lds {
  static constexpr int PADH = KS == 3 ? DIL : 0, HP = (f16x3::TH + 2 * PADH) * (f16x3::TW + 2 * PADH);
  static constexpr int PW = f16x3::TW + 4, PH = f16x3::TH + 4;   // image patch: halo of the halo
  static constexpr int As = 0;                                    // [HP][ROWB]
  static constexpr int Bs = HP * f16x3::ROWB;                     // [2][KS][BN][ROWB]
  static constexpr int patch = Bs + 2 * KS * BN * f16x3::ROWB;    // FUSE1: [3][PH][PW] floats
  static constexpr int w1s = patch + 3 * PH * PW * 4;             // FUSE1: [27][64] floats
  static constexpr int b1s = w1s + 27 * 64 * 4;                   // FUSE1: [64] floats
  static constexpr int Cs = 0;                                    // epilogue: [256][BN + CS_PAD] floats
  static constexpr int CS_B = 256 * (BN + CS_PAD) * 4;
  static constexpr size_t bytes = (size_t)(patch > CS_B ? patch : CS_B) + (FUSE1 ? b1s + 64 * 4 - patch : 0);
  static_assert(Cs + CS_B <= bytes && (!FUSE1 || b1s + 64 * 4 <= bytes), "every region inside the allocation");
};

// producer / consumer kernel of the fused first pair (conv_f16x3_pc.h), Cin = Cout = 64
struct PcLds {
  static constexpr int BN = 64;
  static constexpr int PW = f16x3::TW + 4, PH = f16x3::TH + 4;
  static constexpr int HPP = (f16x3::HP + 31) / 32 * 32;   // 352: tile rows padded to whole 32-row MFMA tiles
  // HALO TILES (round 5): a pixel is ROWB = 144 B ([hi 32 | lo 32 | 16 B]: eight consecutive pixels of a row fall on eight
  // different 16-byte bank groups), a halo ROW is 18 pixels + 96 B = 2 688 B = 128 mod 256: the 16 lanes of a
  // ds_read_b128 group are 8 pixels of row y and 8 of row y + 1 (row_to_pixel), and with the plain 18 x 144 = 2 592 B rows
  // (32 mod 256) the second row's groups fell two slots beside the first's -- a 2-way conflict on every A-fragment read
  // (SQ_LDS_BANK_CONFLICT 0.32 of the kernel's LDS cycles in rounds 3-4, and the consumers' K loop is LDS-bound: 8 KiB of
  // fragments per 12 MFMAs and wave).  The 3.4 KB the padding costs come from the weight rows (below).
  static constexpr int AROW = f16x3::HTW * f16x3::ROWB + 96;   // 2 688 B per halo row
  static constexpr int AT_B = f16x3::HTH * AROW;               // 48 384 B per halo tile
  static_assert(AROW % 256 == 128, "consecutive halo rows on complementary halves of the bank row");
  // WEIGHT ROWS are 128 B without padding (the 8-wave kernel's pack has 144-byte rows): the eight 16-byte pieces of cout
  // row r -- hi k 0-7 .. 24-31, lo k 0-7 .. 24-31 -- are rotated by (r >> 1) mod 8 (pack_conv_weights_split16r), so the 16
  // lanes of a B-fragment read (16 consecutive rows, one logical piece) still cover all 16 bank groups; a tap slab is
  // 8 KiB = 8 DMA pieces, a stage 24 = six rounds of the four producer waves with no ragged one.
  static constexpr int WROWB = 128;
  static constexpr int PATCH_DW = 3 * PH * PW + 8;   // (+ 8 dwords: half-wave 1's zero-weight slots read one element past a tap)
  static constexpr int PC_TABN = 300;                // tiles a block of the persistent walk can hold in its table
  static constexpr int As0 = 0;                            // [HTH][AROW] channels  0..31 of conv1_1's output
  static constexpr int As1 = AT_B;                         // [HTH][AROW] channels 32..63
  static constexpr int Bs = 2 * AT_B;                      // [2][3][BN][WROWB]
  static constexpr int patch = Bs + 2 * 3 * BN * WROWB;    // [PATCH_DW] the image patch, already split
  static constexpr int valid = patch + PATCH_DW * 4;       // [HPP] bytes: halo pixel inside the image?
  static constexpr int bias2L = valid + HPP;               // [BN] floats: conv1_2's biases
  static constexpr int w1L = bias2L + BN * 4;              // 8192 B: conv1_1's weight fragments
  static constexpr int b1L = w1L + 8192;                   // [64] floats: conv1_1's biases
  static constexpr int ctrL = b1L + 64 * 4;                // [4] words: the row-tile counter, halo_inside
  static constexpr int geoL = ctrL + 4 * 4;                // [16] words: the next tile's geometry
  static constexpr int tabL = geoL + 16 * 4;               // [PC_TABN] words: the tiles this block walks
  static constexpr size_t bytes = tabL + PC_TABN * 4;
};

// The dual-tile 4-wave family's planar halo tiles and weight slabs (conv_f16x3_w4d.h; shared by the three-heads kernel):
// plane q (hi k 0-7 | hi k 8-15 | lo k 0-7 | lo k 8-15) holds one 16-byte piece per halo pixel, rows of 24 pixels (384 B
// = 8 sixteen-byte slots mod 16, so the two pixel rows a ds_read_b128 lane group touches land on complementary halves of
// the 256-B bank row), planes 32 B apart mod 128 (the 8-lane groups of the parking ds_write_b128 -- 2 pixels x 4 planes --
// cover all 32 banks).  HTH = halo rows of the tile.
template <int HTH_>
struct W4dTile {
  static constexpr int HTH = HTH_, BN = 128;
  static constexpr int PROW = 24 * 16;                // 384 B per halo-tile row of a plane (18 pixels used at dilation 1)
  static constexpr int PLANE = HTH * PROW + 32;       // 6 944 B (16-row tiles) / 3 872 B (8-row tiles) at dilation 1
  static constexpr int AS_B = 4 * PLANE;              // 27 776 B / 15 488 B per halo tile
  static constexpr int WROWB = 64;                    // weight rows: no padding, the 16-byte pieces rotated by row / 4
  static constexpr int SLAB_B = BN * WROWB;           // 8 192 B per tap slab
};
// conv_mfma_f16x3_w4d_kernel<.., MT, NTILE, .., DIL> and its slim form (MT 2, NTILE 1, DIL 1, SLIM)
template <int MT, int NTILE, int DIL, bool SLIM>
struct W4dLds : W4dTile<4 * MT + 2 * DIL> {
  using T = W4dTile<4 * MT + 2 * DIL>;
  static constexpr int NB_B = NTILE * T::AS_B;                        // one buffer set (the tiles of one chunk)
  static constexpr int As = 0;                                        // [2 buffer sets][NTILE][4 planes][HTH][24 px][16 B]; SLIM: one set
  static constexpr int Bs = (SLIM ? 1 : 2) * NB_B;                    // [2 buffers][3 taps][BN][64 B]; SLIM: a ring of [4 slabs][BN][64 B]
  static constexpr int biasL = Bs + (SLIM ? 4 : 2 * 3) * T::SLAB_B;   // [BN] floats
  static constexpr size_t bytes = biasL + T::BN * 4;
};
// conv_mfma_f16x3_heads3_kernel: one 8 x 16 tile cut for dilation 4 = 16 halo rows of exactly 24 pixels, two buffer sets
struct H3Lds : W4dTile<16> {
  static constexpr int As = 0;                        // [2 buffer sets][4 planes][HTH][24 px][16 B]
  static constexpr int Bs = 2 * AS_B;                 // [2 buffers][3 taps][BN][64 B]
  static constexpr int biasL = Bs + 2 * 3 * SLAB_B;   // [BN] floats
  static constexpr size_t bytes = biasL + BN * 4;
};

// 1x1 GEMM kernel (conv_f16x3_k1.h): 3 x 32 KiB of activations + 2 x 32 KiB of weights = the 160 KiB of a CU; the fp32
// epilogue stages each wave's 32 pixels x 256 couts through the idle buffers
struct K1Lds {
  static constexpr int BN = 256, PXB = 256, WROWB = 64;
  static constexpr int SLAB_B = BN * WROWB;           // 16 KiB: one 16-channel slab of the block's couts
  static constexpr int BUF_B = 2 * SLAB_B;            // a 32-channel chunk of weights
  static constexpr int ABUF_B = PXB * 128;            // a 32-channel chunk of the block's pixels
  static constexpr int EROW = BN * 4 + 16;            // epilogue rows of 1 KiB + 16 B
  static constexpr int As = 0;                        // [3 buffers][256 pixels][128 B]
  static constexpr int Bs = 3 * ABUF_B;               // [2 buffers][2 slabs][BN][64 B]
  static constexpr int Ew = 0;                        // epilogue: [4 waves][32 pixels][EROW]
  static constexpr int EW_B = 32 * EROW;              // ... per wave
  static constexpr size_t bytes = Bs + 2 * BUF_B;
  static_assert(Ew + 4 * EW_B <= bytes, "the epilogue staging inside the allocation");
};

// The slim form shares a CU three ways (conv_f16x3.hip: w4_slim)
constexpr size_t W4_SLIM_LDS_MAX = 163840 / 3 / 128 * 128;   // 54 528 B
static_assert(W4dLds<2, 1, 1, true>::bytes <= W4_SLIM_LDS_MAX, "the slim form does not fit a third of the LDS");

// ---- the totals of every instantiated layout, as the planner used to add them up by hand
static_assert(F32Lds<3, 1, 128, 8>::bytes == 62784 && F32Lds<3, 2, 128, 8>::bytes == 71424 && F32Lds<3, 4, 128, 8>::bytes == 92160, "");
static_assert(F32Lds<3, 1, 64, 16>::bytes == 65088 && F32Lds<3, 2, 64, 16>::bytes == 76032 && F32Lds<3, 4, 64, 16>::bytes == 101376, "");
static_assert(F32Lds<1, 0, 128, 8>::bytes == 55296 && F32Lds<1, 0, 64, 16>::bytes == 55296, "");
static_assert(W8Lds<128, 1, 3, false>::bytes == 157248 && W8Lds<128, 1, 1, false>::bytes == 147456, "");
static_assert(W8Lds<64, 1, 3, false>::bytes == 101952 && W8Lds<64, 2, 3, false>::bytes == 112896 && W8Lds<64, 4, 3, false>::bytes == 138240, "");
static_assert(W8Lds<64, 1, 1, false>::bytes == 81920 && W8Lds<64, 1, 3, true>::bytes == 113920, "");
static_assert(PcLds::bytes == 161088, "");
static_assert(W4dLds<4, 1, 1, false>::bytes == 105216 && W4dLds<4, 2, 1, false>::bytes == 160768, "");
static_assert(W4dLds<2, 1, 1, false>::bytes == 80640 && W4dLds<2, 2, 1, false>::bytes == 111616, "");
static_assert(W4dLds<4, 1, 2, false>::bytes == 111360 && W4dLds<4, 1, 4, false>::bytes == 123648, "");
static_assert(W4dLds<2, 1, 1, true>::bytes == 48768, "");
static_assert(H3Lds::bytes == 99072, "");
static_assert(K1Lds::bytes == 163840, "");

}  // namespace shf
