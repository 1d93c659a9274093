// gemm_plain_ws.hip — the PNC_A_PLAIN instantiations of the GEMM kernel template WITH the weight part (gemm_dispatch.h: dispatch_plain;
// pnc_gemm_wsplit_f16: the fp16 lo plane of the weights beside the parameter block, gemm_kernel.h: gemm_glds_ws_kernel).
#include "gemm_dispatch.h"

template int pnc_gemm::dispatch_plain<true>(const PncGemmParams&, unsigned, hipStream_t, bool*, const void*);

PNC_DEFINE_TU_COLLECT(gemm_plain_ws)
