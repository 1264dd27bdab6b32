// Device-resident blob input (shf_blob_load_device and shf_blob_load_device_group, net_api.cpp): a level that is already in HBM goes into a net input
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

// The same copy for the same input blob of up to 16 nets in ONE launch (shf_blob_load_device_group): an image's pyramid is
// ten such loads, seven of them launch-bound.  The member table travels by value in the kernel argument (like the
// convolutions' ConvK members); a block finds its member from the prefix of block counts -- a linear walk over at most 16
// scalars --, then its (column block, row block, plane) inside the member.  A block is 2^bw_log2 column groups wide and
// 256 >> bw_log2 rows high, so a narrow level still fills its waves.  Within a member it is the work of the two kernels
// above: a thread per four destination columns with one float4 store and scalar reads, or -- a member whose W % 4 != 0 or
// whose destination is unaligned -- a thread per destination element.  The form is a flag of the member, and a block
// belongs to one member: the branch is uniform over the block.  Every destination element is written, padding as +0.0f.
__global__ void __launch_bounds__(256) pad_flip_nchw_group_kernel(const shf::PadFlipGroup g) {
  const unsigned b = blockIdx.x;
  int mi = 0;
  while (mi + 1 < g.n && b >= g.start[mi + 1]) ++mi;
  const shf::PadFlipMember& m = g.m[mi];
  unsigned local = b - g.start[mi];
  const unsigned cb = local % m.bx;
  local /= m.bx;
  const unsigned rb = local % m.by;
  const size_t plane = local / m.by;                 // < planes: the member has bx * by * planes blocks
  const int col = (int)(cb << m.bw_log2) + (int)(threadIdx.x & ((1u << m.bw_log2) - 1u));
  const int y = (int)(rb * (256u >> m.bw_log2)) + (int)(threadIdx.x >> m.bw_log2);
  if (y >= m.H) return;
  const int h = m.h, w = m.w, W = m.W, flip = m.flip;
  const float* row = m.src + (plane * (size_t)h + (size_t)y) * (size_t)w;   // (read only when y < h)
  float* orow = m.dst + (plane * (size_t)m.H + (size_t)y) * (size_t)W;
  if (m.vec) {
    const int x = 4 * col;
    if (x >= W) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y < h) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < w) v[j] = row[flip ? w - 1 - (x + j) : x + j];
    }
    *reinterpret_cast<float4*>(orow + x) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    const int x = col;
    if (x >= W) return;
    float v = 0.f;
    if (y < h && x < w) v = row[flip ? w - 1 - x : x];
    orow[x] = v;
  }
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

int launch_pad_flip_nchw_group(const PadFlipUnit* u, int n, hipStream_t s) {
  if (!u || n < 1 || n > kPadFlipMaxGroup) {
    set_error("pad_flip_nchw group: 1.." + std::to_string(kPadFlipMaxGroup) + " members");
    return -1;
  }
  PadFlipGroup g;
  g.n = n;
  unsigned long long total = 0;
  for (int i = 0; i < n; ++i) {
    const PadFlipUnit& a = u[i];
    const std::string who = "pad_flip_nchw group: member " + std::to_string(i) + ": ";
    if (!a.src || !a.dst || a.n < 1 || a.c < 1 || a.h < 1 || a.w < 1 || a.h > a.H || a.w > a.W || (a.flip != 0 && a.flip != 1)) {
      set_error(who + "bad geometry (" + std::to_string(a.n) + ", " + std::to_string(a.c) + ", " + std::to_string(a.h) + ", " +
                std::to_string(a.w) + ") -> (" + std::to_string(a.H) + ", " + std::to_string(a.W) + ")");
      return -1;
    }
    const long long planes = (long long)a.n * a.c;
    if (a.H > (1 << 30) || a.W > (1 << 30) || planes > 0x7fffffffLL) {
      set_error(who + std::to_string(a.H) + " rows x " + std::to_string(a.W) + " columns x " + std::to_string(planes) +
                " planes exceed the launch limits");
      return -1;
    }
    PadFlipMember& m = g.m[i];
    m.src = a.src; m.dst = a.dst;
    m.h = a.h; m.w = a.w; m.H = a.H; m.W = a.W;
    m.flip = a.flip; m.planes = (int)planes;
    m.vec = a.W % 4 == 0 && ((uintptr_t)a.dst & 15) == 0 ? 1 : 0;
    const unsigned cols = m.vec ? (unsigned)a.W / 4 : (unsigned)a.W;   // column groups, or columns
    m.bw_log2 = 0;
    while (m.bw_log2 < 8 && (1u << m.bw_log2) < cols) ++m.bw_log2;
    const unsigned bw = 1u << m.bw_log2, rpb = 256u >> m.bw_log2;
    m.bx = (cols + bw - 1) / bw;
    m.by = ((unsigned)a.H + rpb - 1) / rpb;
    g.start[i] = (unsigned)total;
    total += (unsigned long long)m.bx * m.by * (unsigned long long)planes;
    // one flat grid of at most 2^31 - 1 blocks: a larger total is refused, never wrapped
    if (total > 0x7fffffffULL) {
      set_error("pad_flip_nchw group: the members up to " + std::to_string(i) + " need " + std::to_string(total) +
                " blocks, the launch limit is 2147483647");
      return -1;
    }
  }
  for (int i = n; i <= kPadFlipMaxGroup; ++i) g.start[i] = (unsigned)total;
  pad_flip_nchw_group_kernel<<<dim3((unsigned)total), 256, 0, s>>>(g);
  SHF_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace shf
