// gemm_conv1d.hip — the PNC_A_CONV1D_T instantiations of the GEMM kernel template (gemm_dispatch.h: dispatch_conv1d), without the weight part.
#include "gemm_dispatch.h"

template int pnc_gemm::dispatch_conv1d<false>(const PncGemmParams&, unsigned, hipStream_t, const void*);

PNC_DEFINE_TU_COLLECT(gemm_conv1d)
