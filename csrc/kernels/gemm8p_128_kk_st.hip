// tiresias_amd — one production gemm8p variant per translation unit (gemm8p.h):
// the 128x128 tile, K-major A and B, BatchNorm statistics in the epilogue.
#include "tam/gemm8p.h"

namespace tam {
TAM_P8_ST_INST(128, 128, 2)
}  // namespace tam
