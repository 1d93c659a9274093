// gemm_conv1d_ws.hip — the PNC_A_CONV1D_T instantiations of the GEMM kernel template WITH the weight part (gemm_dispatch.h:
// dispatch_conv1d; pnc_gemm_wsplit_f16).
#include "gemm_dispatch.h"

template int pnc_gemm::dispatch_conv1d<true>(const PncGemmParams&, unsigned, hipStream_t, const void*);

PNC_DEFINE_TU_COLLECT(gemm_conv1d_ws)
