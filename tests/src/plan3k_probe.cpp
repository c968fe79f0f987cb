// plan3k_probe -- prints the walk the volume family's planner chooses for a window of a given radius (tests/test_ssim3k_cpu.py).
//
// Reads rows "radius width height depth count cus" from stdin and prints one row "tiles_x tiles_y cells_z chunk_slices chunks max_count"
// each, from plan3k (ssim3k_kernels.h: plan3f with 2 * radius warm-up slices) and ssim3f_max_count of the project's kernel object.  Host
// arithmetic only: no HIP call, no device.
#include <cstdio>

#include "ssim3k_kernels.h"

int main()
{
    unsigned radius, width, height, depth, count;
    int cus;
    while (scanf("%u %u %u %u %u %d", &radius, &width, &height, &depth, &count, &cus) == 6) {
        const ssim_hip::Geometry3F g = ssim_hip::plan3k(radius, width, height, depth, count, cus);
        printf("%u %u %u %u %u %u\n", g.tiles_x, g.tiles_y, g.cells_z, g.chunk_slices, g.chunks, ssim_hip::ssim3f_max_count(width, height, depth));
    }
    return feof(stdin) ? 0 : 2;
}
