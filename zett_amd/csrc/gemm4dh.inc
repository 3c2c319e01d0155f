// gemm4dh.inc — body of gemm4dh_<type>.hip: the 128x256 HALF instantiations of the four-wave direct-to-LDS tile (gemm4d.hip.h)
// for one 16-bit operand type (ZETT_GEMM_T), in their own translation unit so that they compile beside the full tiles.
#include <hip/hip_runtime.h>

#include "gemm.hip.h"
#include "gemm_tile.hip.h"
#include "gemm4d.hip.h"

namespace zett {

hipError_t launch_gemm_4d_half(const GemmArgs<ZETT_GEMM_T>& g, hipStream_t stream, int mode) {
    return launch_gemm4d_mode<ZETT_GEMM_T, true>(g, stream, mode);
}

hipError_t launch_gemm_4d_half_dst(const GemmArgs<ZETT_GEMM_T>& g, hipStream_t stream, int mode) {
    return launch_gemm4d_dst_mode<ZETT_GEMM_T, true>(g, stream, mode);
}

}  // namespace zett
