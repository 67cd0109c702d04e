// GEMM tile family instantiations (see net_gemm_kernel.hpp); one
// translation unit per family so hipcc compiles them in parallel.
#include "net_gemm_kernel.hpp"

namespace s3gemm {
// 32x32x16 MFMA: large tiles and K tile 128
int launch_t2(int tile, const GemmP& p, hipStream_t st) {
  switch (tile) {
#define S3_TILE_UNIT 2
#define S3_TILE_GEMM(id, tail, tuner, ...) case id: return launch<__VA_ARGS__>(p, st);
#include "net_gemm_tiles.def"
  }
  return kNotMine;
}
int sat_t2(int reset) { return read_sat(reset); }
}  // namespace s3gemm
