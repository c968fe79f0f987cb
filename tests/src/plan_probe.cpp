// plan_probe -- prints the strip height the sample families' planners choose (tests/test_sample_plan_cpu.py).
//
// Reads rows "family radius width height count cus" from stdin (family: ssim16, ssimf, ssimh, ssimk, msssimf; radius is read for every
// family and used by ssimk alone) and prints one row "cell_rows strip_rows strips_x strips_y cells_y" each (cell_rows 0 for
// msssimf, whose launcher exposes the cells of a scale and not their height), from plan16 / planf / planh / plank /
// strip_rows_of and msf_cells of the project's kernel objects.  Host arithmetic only: no HIP call, no device.
#include <cstdio>
#include <cstring>

#include "msssimf_kernels.h"
#include "ssim16_kernels.h"
#include "ssimf_kernels.h"
#include "ssimh_kernels.h"
#include "ssimk_kernels.h"

int main()
{
    char family[16];
    unsigned radius, width, height, count;
    int cus;
    while (scanf("%15s %u %u %u %u %d", family, &radius, &width, &height, &count, &cus) == 6) {
        unsigned cell_rows, strip_rows, strips_x, strips_y, cells_y;
        if (!strcmp(family, "ssim16")) {
            const ssim_hip::Geometry16 g = ssim_hip::plan16(width, height, count, cus);
            cell_rows = g.cell_rows; strip_rows = g.strip_rows; strips_x = g.strips_x; strips_y = g.strips_y; cells_y = g.cells_y;
        } else if (!strcmp(family, "ssimf")) {
            const ssim_hip::GeometryF g = ssim_hip::planf(width, height, count, cus);
            cell_rows = g.cell_rows; strip_rows = g.strip_rows; strips_x = g.strips_x; strips_y = g.strips_y; cells_y = g.cells_y;
        } else if (!strcmp(family, "ssimh")) {
            const ssim_hip::GeometryH g = ssim_hip::planh(width, height, count, cus);
            cell_rows = g.cell_rows; strip_rows = g.strip_rows; strips_x = g.strips_x; strips_y = g.strips_y; cells_y = g.cells_y;
        } else if (!strcmp(family, "ssimk")) {
            const ssim_hip::GeometryF g = ssim_hip::plank(radius, width, height, count, cus);
            cell_rows = g.cell_rows; strip_rows = g.strip_rows; strips_x = g.strips_x; strips_y = g.strips_y; cells_y = g.cells_y;
        } else if (!strcmp(family, "msssimf")) {
            // launch_msssimf's own arithmetic around strip_rows_of for one scale
            strip_rows = ssim_hip::strip_rows_of(width, height, count, cus);
            cell_rows = 0;
            cells_y = (unsigned)ssim_hip::msf_cells(1, height, 0);
            strips_x = (width + ssim_hip::kSFStripW - 1) / ssim_hip::kSFStripW;
            strips_y = (height + strip_rows - 1) / strip_rows;
        } else {
            fprintf(stderr, "plan_probe: unknown family %s\n", family);
            return 2;
        }
        printf("%u %u %u %u %u\n", cell_rows, strip_rows, strips_x, strips_y, cells_y);
    }
    return feof(stdin) ? 0 : 2;
}
