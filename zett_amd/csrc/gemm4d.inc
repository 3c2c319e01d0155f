// gemm4d.inc — body of gemm4d_<type>.hip: the four-wave direct-to-LDS tile for one 16-bit operand type (ZETT_GEMM_T).
#include <hip/hip_runtime.h>

#include "gemm.hip.h"
#include "gemm_tile.hip.h"
#include "gemm4d.hip.h"
#include "gemm_launch.hip.h"

namespace zett {

hipError_t launch_gemm_4d(const GemmArgs<ZETT_GEMM_T>& g, hipStream_t stream, bool generic_epilogue) {
    return launch_gemm4d<ZETT_GEMM_T>(g, stream, generic_epilogue);
}

int gemm_4d_dst_mode(const GemmArgs<ZETT_GEMM_T>& g) { return gemm4d_dst_mode<ZETT_GEMM_T>(g); }

int gemm_4d_launch_mode(const GemmArgs<ZETT_GEMM_T>& g, bool generic_epilogue) { return gemm4d_launch_mode<ZETT_GEMM_T>(g, generic_epilogue); }

}  // namespace zett
