// hipFFT for the library (field.hip): the one loader (dlopen at first use, like RCCL) and the plan cache, shared by the
// volume synthesis, the power spectra (field.hip) and the Fresnel propagation (fresnel.hip).
#pragma once
#include <hipfft/hipfft.h>

// the one check of a hipfftResult: the entry's name, the call's text and the result code
#define SR_FFT(who, call)                                                                                        \
  do {                                                                                                           \
    const hipfftResult r_ = (call);                                                                              \
    if (r_ != HIPFFT_SUCCESS) return sr::fail(SR_ERR_HIP, "%s: %s failed: hipfftResult %d", who, #call, (int)r_); \
  } while (0)

namespace sr {

struct Fft {
  void *h = nullptr;
  hipfftResult (*Plan3d)(hipfftHandle *, int, int, int, hipfftType) = nullptr;
  hipfftResult (*Plan2d)(hipfftHandle *, int, int, hipfftType) = nullptr;
  hipfftResult (*Plan1d)(hipfftHandle *, int, hipfftType, int) = nullptr;
  hipfftResult (*SetStream)(hipfftHandle, hipStream_t) = nullptr;
  hipfftResult (*ExecZ2Z)(hipfftHandle, hipfftDoubleComplex *, hipfftDoubleComplex *, int) = nullptr;
  hipfftResult (*Destroy)(hipfftHandle) = nullptr;
};

int fft_lib(Fft **out);
// Z2Z plan of rank 1-3 over (n0[, n1[, n2]]) (C order), created at first use and kept for the life of the process
int fft_plan(Fft *F, int rank, int n0, int n1, int n2, hipfftHandle *out);

}  // namespace sr
