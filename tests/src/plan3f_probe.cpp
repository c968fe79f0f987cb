// plan3f_probe -- prints the walk the volume family's planner chooses (tests/test_ssim3f_plan_cpu.py).
//
// Reads rows "width height depth count cus" from stdin and prints one row "tiles_x tiles_y cells_z chunk_slices chunks max_count" each,
// from plan3f and ssim3f_max_count of the project's kernel object.  Host arithmetic only: no HIP call, no device.
#include <cstdio>

#include "ssim3f_kernels.h"

int main()
{
    unsigned width, height, depth, count;
    int cus;
    while (scanf("%u %u %u %u %d", &width, &height, &depth, &count, &cus) == 5) {
        const ssim_hip::Geometry3F g = ssim_hip::plan3f(width, height, depth, count, cus);
        printf("%u %u %u %u %u %u\n", g.tiles_x, g.tiles_y, g.cells_z, g.chunk_slices, g.chunks, ssim_hip::ssim3f_max_count(width, height, depth));
    }
    return feof(stdin) ? 0 : 2;
}
