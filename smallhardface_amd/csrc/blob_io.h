// Launcher of the device-resident blob input kernel (blob_io.hip), called by shf_blob_load_device (net_api.cpp).
#pragma once
#include "shf_internal.h"

namespace shf {

// a level already on the device into a net input: src (n, c, h, w) fp32 NCHW -> dst (n, c, H, W), mirrored along x when
// flip, +0.0f below h / right of w; EVERY destination element is written.  Refuses (message, nothing launched) bad geometry
// and shapes whose grid (column groups, H, n * c) exceeds the launch limits.
int launch_pad_flip_nchw(const float* src, int n, int c, int h, int w, float* dst, int H, int W, int flip, hipStream_t s);

}  // namespace shf
