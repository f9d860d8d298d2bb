// tiresias_amd — one production gemm8p variant per translation unit (gemm8p.h):
// the 256x256 tile, K-major A and B, BatchNorm statistics in the epilogue.
#include "tam/gemm8p.h"

namespace tam {
TAM_P8_ST_INST(256, 256, 4)
}  // namespace tam
