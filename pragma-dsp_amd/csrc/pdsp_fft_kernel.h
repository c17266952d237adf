// pdsp_fft_kernel.h -- every FFT kernel family at once (the dispatchers and the kernel benches take them all).
#pragma once

#include "pdsp_fft_core.h"
#include "pdsp_packed.h"
#include "pdsp_peaks.h"
#include "pdsp_fft_rows_kernel.h"
#include "pdsp_spectrum_kernel.h"
#include "pdsp_multipass_kernel.h"
#include "pdsp_elementwise_kernel.h"
