// Split-fp16 convolution, the dual-tile 4-wave family: every 3x3 / dilation-1 layer with Cin >= 64 and Cout % 128 == 0.
// (part of the one translation unit conv_f16x3.hip: see its header for the arithmetic and the kernel map)
#pragma once
#include "conv_common.h"

#include "conv_f16x3_types.h"

namespace shf {

// DUAL-TILE form of the 4-wave kernel: a block computes TWO 16x16-pixel tiles (consecutive in the launch's tile order)
// x 128 couts and every weight slab it fetches serves both -- the weights' way from L2 to LDS is what this power-limited
// kernel pays most for after the MFMAs themselves (halving it is worth 15 %).  What makes room for the second
// tile's accumulators is ONE accumulator per output instead of two: the low parts are kept UNSCALED in LDS
// (lo = fp16(x - hi); the split activation format of HBM keeps its 2^11 -- the halo staging multiplies it away; the
// weights come from their own pack, pre-scaled by a power of two: pack_conv_weights_split16h), so hi*hi, hi*lo and
// lo*hi have one scale and share a register (v_mfma_f32_32x32x16_f16 honours fp16 subnormals: tools/mfma_denorm.hip;
// end-to-end error of the scheme: tools/single_acc_study.py).  What makes room for the second halo tile's hand-over
// registers is a CHUNK of 16 input channels instead of 32: a stage is still one kernel row of a chunk = 144 MFMAs per
// wave (3 taps x 1 k-step x 2 tiles x 24), its three weight slabs are 30 KB instead of 55, a halo tile 30 KB instead
// of 48, and a hand-over moves 2 x 6 pieces per thread.  The six half-steps of a stage (tap kx, tile t) are
// software-pipelined like the six k-steps of the single-tile kernel: while (kx, t) runs, the A fragments of the next
// (kx, t) -- and, on even half-steps, the B fragments of tap kx + 1 -- are read.
//
// HALO TILES ARE DOUBLE-BUFFERED (round 3): with one buffer per tile the hand-over was a serial section -- barrier,
// convert + park 12 pieces, barrier, first fragment reads -- that cost the dominant launch 7.6 % with the matrix pipe
// idle (tools/experiments/w4d_power_ablation.sh: no_halo).  Chunk c + 1's pieces are now requested during kernel row
// 1 of chunk c and converted + parked into the OTHER buffer pair under the MFMAs of kernel row 2, two pieces per
// half-step; the next stage's barrier -- which the weights need anyway -- publishes them.  Four halo tiles fit in
// 160 KB because the layout is PLANAR, without per-row padding: plane q (hi k 0-7 | hi k 8-15 | lo k 0-7 | lo k 8-15)
// holds one 16-byte piece per halo pixel, rows of 24 pixels (384 B = 8 sixteen-byte slots mod 16, so the two pixel
// rows a ds_read_b128 lane group touches land on complementary halves of the 256-B bank row), planes 32 B apart
// mod 128 (the 8-lane groups of the parking ds_write_b128 -- 2 pixels x 4 planes -- cover all 32 banks).  Every
// fragment address is lane offset + immediate: tap kx = +16 B, kernel row = +384 B, lo = +2 planes.
// DIL (round 4): the dilated shared-weight heads (dilation 2 / 4, Cin = Cout = 128) run here too, as single 16-row tiles:
// the halo tile is (16 + 2 DIL)^2 pixels -- 20 or 24 per row, inside the 24-pixel plane rows --, a tap is DIL pixels / DIL
// plane rows further, nothing else changes (111 360 / 123 648 B of LDS).  They used to take the 8-wave kernel's 64-cout form (a
// fragment read per MFMA: 0.29 issued).
// SLIM (single 8-row tiles at dilation 1, the short-K layers): the same block in at most a third of a CU -- ONE halo
// buffer and a RING of four tap slabs instead of two buffer sets and the 2 x 3 weight double buffer: 15 488 + 32 768 +
// 512 = 48 768 B, at most 168 registers, so that THREE blocks share a CU and a block's
// prologue and epilogue run under the K loops of two others instead of one.  The K loop walks TAPS, not stages: before
// tap s every wave waits for its pieces of slab s + 1 and for its own LDS traffic, then the block's barrier -- which
// publishes slab s + 1 and RELEASES slab s (its fragments are in registers by then) --, then the fragments of tap s + 1
// are read and slab s + 4 is requested into slab s's slot, all under the MFMAs of tap s.  Two slabs = four DMA pieces per
// wave stay in flight across each barrier: vmcnt(4).  The halo buffer is handed over at the last tap of a chunk: that
// tap's fragments are in registers at its barrier, so chunk c + 1's pieces (requested at tap 3) are converted and parked
// under its MFMAs and the next tap's barrier publishes them; only the first fragment read of a chunk is not covered.
// Per output the operations and their order are those of every other form.
template <bool IN_SPLIT, int MT_, int NTILE, int NP = 3, bool BF = false, int DIL = 1>
__global__ __launch_bounds__(256) void conv_mfma_f16x3_w4d_kernel(ConvK p) {
  constexpr bool SLIM = false;
#include "conv_f16x3_w4d_body.h"
}

// The slim form is a kernel of its own name, so that every other form keeps its code and its name (the profiles and the
// profiler classes are keyed by them); three waves per SIMD bound its registers at 168.
template <bool IN_SPLIT, int NP = 3, bool BF = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void conv_mfma_f16x3_w4d_slim_kernel(ConvK p) {
  constexpr int MT_ = 2, NTILE = 1, DIL = 1;
  constexpr bool SLIM = true;
#include "conv_f16x3_w4d_body.h"
}

}  // namespace shf
