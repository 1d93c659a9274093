// gemm_conv3x3_ws.hip — the PNC_A_CONV3X3 instantiations of the GEMM kernel template WITH the weight part (gemm_dispatch.h:
// dispatch_conv3x3; pnc_gemm_wsplit_f16).
#include "gemm_dispatch.h"

template int pnc_gemm::dispatch_conv3x3<true>(const PncGemmParams&, unsigned, hipStream_t, const void*);

PNC_DEFINE_TU_COLLECT(gemm_conv3x3_ws)
