// gemm_bf16.hip — the bf16 instantiation of the GEMM kernel family (gemm_kernels.h), the bf16-only x3 split epilogues among them
#include "gemm_kernels.h"

template void gemm_launch<BF16>(const GemmArgs&, const GemmLaunch&, hipStream_t);
template void gemm_launch_name<BF16>(const GemmLaunch&, char*, size_t);
