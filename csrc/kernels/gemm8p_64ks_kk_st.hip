// tiresias_amd — one production gemm8p variant per translation unit (gemm8p.h):
// the 64x128 tile with its K range split over two wave groups of one block,
// K-major A and B, BatchNorm statistics in the epilogue.
#include "tam/gemm8p.h"

namespace tam {
TAM_P8_KS2_ST_INST(64, 128, 2)
}  // namespace tam
