// The fixed-shape row transform (zfft_rows.hip): whole, contiguous aperture rows in one resident run, 8 or 16
// residues, two bins per thread.  zfft.hip zfft_run takes it where the call's own arguments show that shape
// (zfft_core.h rows_kernel_takes) and keeps zfft_kernel for everything else.
#pragma once
#include "common.h"

namespace ml {

// c: a call that rows_kernel_takes() accepts; pad1: the in-place layout's padding, grid and lds_bytes as zfft_run
// found them for zfft_kernel (the same exchange buffer and twiddle table, the same rows per workgroup)
int zfft_rows_run(hipStream_t stream, const ZfftCall &c, int pad1, int grid, size_t lds_bytes);

}  // namespace ml
