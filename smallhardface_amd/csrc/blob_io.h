// Launchers of the device-resident blob input kernels (blob_io.hip), called by shf_blob_load_device and
// shf_blob_load_device_group (net_api.cpp).
#pragma once
#include "shf_internal.h"

namespace shf {

// a level already on the device into a net input: src (n, c, h, w) fp32 NCHW -> dst (n, c, H, W), mirrored along x when
// flip, +0.0f below h / right of w; EVERY destination element is written.  Refuses (message, nothing launched) bad geometry
// and shapes whose grid (column groups, H, n * c) exceeds the launch limits.
int launch_pad_flip_nchw(const float* src, int n, int c, int h, int w, float* dst, int H, int W, int flip, hipStream_t s);

// ... and the same copy for up to 16 blobs in ONE launch (pad_flip_nchw_group_kernel).  PadFlipUnit is what the caller
// gives per member; PadFlipGroup is the kernel argument the launcher makes of it, passed by value.
constexpr int kPadFlipMaxGroup = 16;
struct PadFlipUnit {
  const float* src;
  float* dst;
  int n, c, h, w, H, W, flip;
};
struct PadFlipMember {
  const float* src;
  float* dst;
  int h, w, H, W;
  int flip, planes;
  int vec;          // 1: a thread per four destination columns (W % 4 == 0, 16-byte aligned dst); 0: a thread per element
  int bw_log2;      // a block is 2^bw_log2 column groups (columns, scalar form) wide and 256 >> bw_log2 rows high
  unsigned bx, by;  // blocks per row of column groups / per plane of rows: the member has bx * by * planes blocks
};
struct PadFlipGroup {
  int n;
  unsigned start[kPadFlipMaxGroup + 1];   // prefix of the members' block counts; start[n ..] = the grid size
  PadFlipMember m[kPadFlipMaxGroup];
};
// Refuses (message naming the member, nothing launched) n outside 1..16, bad geometry, and a total beyond the 2^31 - 1
// blocks of a flat 1-D grid.
int launch_pad_flip_nchw_group(const PadFlipUnit* u, int n, hipStream_t s);

}  // namespace shf
