// GEMM tile family instantiations (see net_gemm_kernel.hpp); one
// translation unit per family so hipcc compiles them in parallel.
#include "net_gemm_kernel.hpp"

namespace s3gemm {
// v_mfma_f32_16x16x32 tiles, 4 waves.  They need the vector epilogue (aligned
// operands); launch<> rejects a launch without it -- no silent fallback to
// another tile, which would change the launch's reduction class
// (ops.reduction_class); the tuner skips the error.
int launch_t4(int tile, const GemmP& p, hipStream_t st) {
  switch (tile) {
#define S3_TILE_UNIT 4
#define S3_TILE_GEMM(id, tail, tuner, ...) case id: return launch<__VA_ARGS__>(p, st);
#include "net_gemm_tiles.def"
  }
  return kNotMine;
}
int sat_t4(int reset) { return read_sat(reset); }
}  // namespace s3gemm
