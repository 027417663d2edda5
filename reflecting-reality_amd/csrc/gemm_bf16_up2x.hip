// bf16 phase forms of tiles 42, 43, 48: the 3x3 conv over a nearest-2x upsampled image as four 2x2 convs in one launch (mf_conv_up2x)
// (tile tables: gemm_16bit_tiles.h, kernel template: gemm_conv_kernel.h, MF_FX_UP)
#include "gemm_16bit_tiles.h"

namespace mfgemm {
bool launch_bf16_up2x(int tile, const GemmArgs& a, dim3 grid, hipStream_t s) { return launch16_up2x<MF_BF16>(tile, a, grid, s); }
}  // namespace mfgemm
