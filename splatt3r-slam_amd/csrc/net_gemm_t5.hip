// GEMM tile family instantiations (see net_gemm_kernel.hpp); one
// translation unit per family so hipcc compiles them in parallel.
#include "net_gemm_kernel.hpp"

namespace s3gemm {
// v_mfma_f32_16x16x32 tiles, continued
int launch_t5(int tile, const GemmP& p, hipStream_t st) {
  switch (tile) {
#define S3_TILE_UNIT 5
#define S3_TILE_GEMM(id, tail, tuner, ...) case id: return launch<__VA_ARGS__>(p, st);
#include "net_gemm_tiles.def"
  }
  return kNotMine;
}
int sat_t5(int reset) { return read_sat(reset); }
}  // namespace s3gemm
