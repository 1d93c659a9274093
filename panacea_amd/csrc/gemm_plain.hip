// gemm_plain.hip — the PNC_A_PLAIN instantiations of the GEMM kernel template (gemm_dispatch.h: dispatch_plain), without the weight part.
#include "gemm_dispatch.h"

template int pnc_gemm::dispatch_plain<false>(const PncGemmParams&, unsigned, hipStream_t, bool*, const void*);

PNC_DEFINE_TU_COLLECT(gemm_plain)
