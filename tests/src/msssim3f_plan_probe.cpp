// msssim3f_plan_probe -- prints the scratch and sub-batch rule of multi-scale SSIM of float32 volumes (tests/test_msssim3f_cpu.py).
//
// Reads rows "width height depth scales cap" from stdin and prints one row "max_count pyramid_floats partials forward_bytes one_grad_bytes
// both_grads_bytes forward_per one_grad_per both_grads_per" each, from the functions of msssim3f_kernels.h in the project's kernel objects
// that the host flow (ssim_volumes_abi.cpp) calls.  Host arithmetic only: no HIP call, no device.
#include <cstdio>

#include "msssim3f_kernels.h"

int main()
{
    unsigned width, height, depth, scales;
    unsigned long long cap;
    while (scanf("%u %u %u %u %llu", &width, &height, &depth, &scales, &cap) == 5) {
        printf("%u %llu %llu", ssim_hip::msssim3f_max_count(width, height, depth),
               (unsigned long long)ssim_hip::ms3_pyramid_floats(width, height, depth, scales),
               (unsigned long long)ssim_hip::ms3_partials(width, height, depth, 1, scales));
        for (int planes = 0; planes <= 2; ++planes)
            printf(" %llu", (unsigned long long)ssim_hip::msssim3f_scratch_bytes(width, height, depth, scales, planes));
        for (int planes = 0; planes <= 2; ++planes)
            printf(" %u", ssim_hip::msssim3f_per_sub_batch(width, height, depth, scales, planes, cap));
        printf("\n");
    }
    return feof(stdin) ? 0 : 2;
}
