// Device-resident blob input (shf_blob_load_device, net_api.cpp): a level that is already in HBM goes into a net input
// without visiting the host -- Blob::set_gpu_data (caffe/src/caffe/blob.cpp:114-121) with forward_net's zero pad
// (lib/test.py:35-38) and detect()'s horizontal flip (:150) folded into the one copy.  Its own translation unit, like
// eval.hip: pre.hip and shf_internal.h are part of the kernel-source hash that ties the committed counter runs to the code
// they were measured on (tools/kernel_hash.py), and nothing measured there changes here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blob_io.h"

namespace {

// Blob::set_gpu_data for a level that is already in HBM (shf_blob_load_device): an (n, c, h, w) fp32 NCHW block lands in
// the (n, c, H, W) blob, mirrored along x when `flip`, the rows below h and the columns right of w written as +0.0f
// (lib/test.py:35-38 np.pad, :150 the [..., ::-1] view).  EVERY destination element is written: the blob's buffer is
// grow-only and still holds the previous unit.  Plain bandwidth: 4 B in, 4 B out per element.
// Vector form: one thread per four destination columns (W % 4 == 0, 16-byte aligned base), one float4 store; the source
// reads stay scalar -- a source row starts at (plane * h + y) * w floats, unaligned for odd w, and runs backwards when flipped.
__global__ void __launch_bounds__(256) pad_flip_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int h,
                                                           int w, int H, int W, int flip) {
  const int x = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
  const int y = blockIdx.y;
  if (x >= W) return;
  const size_t plane = blockIdx.z;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (y < h) {
    const float* row = src + (plane * (size_t)h + (size_t)y) * (size_t)w;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < w) v[j] = row[flip ? w - 1 - (x + j) : x + j];
  }
  float4* o = reinterpret_cast<float4*>(dst + (plane * (size_t)H + (size_t)y) * (size_t)W + (size_t)x);
  *o = make_float4(v[0], v[1], v[2], v[3]);
}

// scalar form (W % 4 != 0 or an unaligned destination): one thread per destination element
__global__ void __launch_bounds__(256) pad_flip_nchw_scalar_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                   int h, int w, int H, int W, int flip) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= W) return;
  const size_t plane = blockIdx.z;
  float v = 0.f;
  if (y < h && x < w) v = src[(plane * (size_t)h + (size_t)y) * (size_t)w + (size_t)(flip ? w - 1 - x : x)];
  dst[(plane * (size_t)H + (size_t)y) * (size_t)W + (size_t)x] = v;
}

}  // namespace

namespace shf {

int launch_pad_flip_nchw(const float* src, int n, int c, int h, int w, float* dst, int H, int W, int flip, hipStream_t s) {
  if (!src || !dst || n < 1 || c < 1 || h < 1 || w < 1 || h > H || w > W || (flip != 0 && flip != 1)) {
    set_error("pad_flip_nchw: bad geometry (" + std::to_string(n) + ", " + std::to_string(c) + ", " + std::to_string(h) +
              ", " + std::to_string(w) + ") -> (" + std::to_string(H) + ", " + std::to_string(W) + ")");
    return -1;
  }
  // grid = (column groups, H, n * c): rows and planes are grid dimensions of at most 65 535 blocks -- refused, never wrapped
  const long long planes = (long long)n * c;
  if (H > 65535 || planes > 65535 || W > (1 << 30)) {
    set_error("pad_flip_nchw: " + std::to_string(H) + " rows x " + std::to_string(planes) +
              " planes (or " + std::to_string(W) + " columns) exceed the launch limits (65535 blocks per grid dimension)");
    return -1;
  }
  const bool vec = W % 4 == 0 && ((uintptr_t)dst & 15) == 0;
  if (vec) {
    const int groups = W / 4;
    const int block = groups >= 256 ? 256 : (groups + 63) / 64 * 64;   // whole waves; a narrow level takes one or two per row
    dim3 grid((groups + block - 1) / block, H, (unsigned)planes);
    pad_flip_nchw_kernel<<<grid, block, 0, s>>>(src, dst, h, w, H, W, flip);
  } else {
    dim3 grid((W + 255) / 256, H, (unsigned)planes);
    pad_flip_nchw_scalar_kernel<<<grid, 256, 0, s>>>(src, dst, h, w, H, W, flip);
  }
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf
