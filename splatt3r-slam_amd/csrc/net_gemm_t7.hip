// GEMM tile family instantiations (see net_gemm_kernel.hpp): 8- and 16-wave
// dense / conv tiles.  The halo-conv measurements (net_gemm_t6.hip) showed
// that at one big-LDS workgroup per CU nothing hides a wave's LDS fragment
// reads and epilogue; these tiles put two waves on every SIMD (8 waves per
// workgroup) or two workgroups on every CU (128x128, 2 stages = 64 KiB).
// (An 8-wave 128x128 32x32x16 tile and a 16-wave 256x256 tile spill at
// these occupancies and are not built.)
#include "net_gemm_kernel.hpp"

namespace s3gemm {
int launch_t7(int tile, const GemmP& p, hipStream_t st) {
  switch (tile) {
#define S3_TILE_UNIT 7
#define S3_TILE_GEMM(id, tail, tuner, ...) case id: return launch<__VA_ARGS__>(p, st);
#include "net_gemm_tiles.def"
  }
  return kNotMine;
}
int sat_t7(int reset) { return read_sat(reset); }
}  // namespace s3gemm
