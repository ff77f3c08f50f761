// ecdsa_key_kernels.hip — batched public-key import and export for gfx950
// (include/lcb_ecdsa_key_gpu.h).  One lane serves one item with
// key_import_one() / key_export_one() of ecdsa_key_math.hpp: no cross-lane
// traffic, no LDS, no atomics, no scratch.  As in the sibling kernels the
// import is v_mad_u64_u32 in a serial chain per lane, so one wave per
// workgroup spreads a small batch over every SIMD.  The exponent of the
// square root is the same in every lane; lanes of different key forms in one
// wave diverge (a compressed key costs some hundred products, every other
// form six), and a lane whose item is refused idles under the mask.
//
// An item whose size is past key_stride reads nothing and gets EINVAL.
#include <hip/hip_runtime.h>

#include "ecdsa_key_internal.hpp"

namespace lcbec {

constexpr int kBlock = 64;
constexpr int kWavesPerSimd = 2;  // as the verification kernel
constexpr int kExportBlock = 256;

__global__ __launch_bounds__(kBlock, kWavesPerSimd) void ecdsa_key_import_kernel(const KeyImportArgs a,
                                                                                  const Curve<kLimbs> c,
                                                                                  const KeyConsts<kLimbs> k) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.count) return;
    uint8_t* out = a.pub + i * (2 * kNumBytes);
    uint8_t* inf = a.infinity ? a.infinity + i : nullptr;
    const uint32_t size = a.sizes ? a.sizes[i] : a.key_size;
    int st = kEinval;
    if (size <= a.key_stride) {  // else no key byte is read
        st = key_import_one<kLimbs>(c, k, a.keys + i * a.key_stride, size,
                                    a.keys_y ? a.keys_y + i * kNumBytes : nullptr, a.le != 0, out, inf);
    } else {
        store_num<kLimbs>(out, small<kLimbs>(0), false);
        store_num<kLimbs>(out + kNumBytes, small<kLimbs>(0), false);
        if (inf) *inf = 0;
    }
    a.status[i] = st;
}

__global__ __launch_bounds__(kExportBlock) void ecdsa_key_export_kernel(const KeyExportArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kExportBlock + threadIdx.x;
    if (i >= a.count) return;
    const bool inf = a.infinity && a.infinity[i] != 0;
    a.out_sizes[i] = key_export_one<kLimbs>(a.pub + i * (2 * kNumBytes), inf, a.compress != 0, a.le != 0,
                                            a.out + i * a.out_stride);
    a.status[i] = 0;
}

void launch_ecdsa_key_import(const KeyImportArgs& a, const Curve<kLimbs>& c, const KeyConsts<kLimbs>& k,
                             hipStream_t s) {
    if (a.count == 0) return;
    const uint64_t blocks = (a.count + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ecdsa_key_import_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a, c, k);
}

void launch_ecdsa_key_export(const KeyExportArgs& a, hipStream_t s) {
    if (a.count == 0) return;
    const uint64_t blocks = (a.count + kExportBlock - 1) / kExportBlock;
    hipLaunchKernelGGL(ecdsa_key_export_kernel, dim3((unsigned)blocks), dim3(kExportBlock), 0, s, a);
}

}  // namespace lcbec
