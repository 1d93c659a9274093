// gemm_conv3x3.hip — the PNC_A_CONV3X3 instantiations of the GEMM kernel template (gemm_dispatch.h: dispatch_conv3x3), without the weight part.
#include "gemm_dispatch.h"

template int pnc_gemm::dispatch_conv3x3<false>(const PncGemmParams&, unsigned, hipStream_t, const void*);

PNC_DEFINE_TU_COLLECT(gemm_conv3x3)
