// DVD_HD marks the arithmetic that the kernels share with their stand-alone CPU restatements (*_host_check.cpp).
#pragma once
#if defined(__HIPCC__)
#define DVD_HD __host__ __device__ __forceinline__
#else
#define DVD_HD inline
#endif
