// Instantiates the reference's header-only test oracle (tests/ssim_naive.h, found through -I<reference>/tests) against THIS
// repository's <rmgr/ssim.h>: oracle/Makefile syntax-checks it into oracle/_ref/header_compat (tests/test_abi_cpu.py reads the result).
#include <ssim_naive.h>
double probe(const rmgr::ssim::GeneralParams& p, double* map)
{ return rmgr::ssim::naive::compute_ssim<double, rmgr::ssim::uint8_t>(p.width, p.height, p.imgA.topLeft, p.imgA.step, p.imgA.stride,
      p.imgB.topLeft, p.imgB.step, p.imgB.stride, map, 1, p.width); }
