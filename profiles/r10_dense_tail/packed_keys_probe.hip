#include <hip/hip_runtime.h>
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__global__ void k(const unsigned *idx, unsigned *out) {
    __shared__ unsigned char blk[4096];
    for (int i = threadIdx.x; i < 4096; i += 64) blk[i] = (unsigned char)(idx[i] >> 3);
    __syncthreads();
    const unsigned L0 = idx[threadIdx.x], L1 = idx[64 + threadIdx.x];
    us2 best = (us2)(0xFFFF);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        us2 c;
        c.x = blk[(L0 >> (8 * s)) & 0xFF];
        c.y = blk[256 + ((L1 >> (8 * s)) & 0xFF)];
        const us2 key = c * (us2)(128) + (us2)((unsigned short)s);
        best = __builtin_elementwise_min(best, key);
    }
    out[threadIdx.x] = min((unsigned)best.x, (unsigned)best.y + 4u);
}
