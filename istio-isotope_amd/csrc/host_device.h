// The __host__ __device__ qualifiers for headers that both hipcc and the host
// compiler read (quantile_rank.h, sketch_bucket.h): the host compiler knows
// neither, and for it they mean nothing.
#pragma once

#if !defined(__HIPCC__)
#if !defined(__host__)
#define __host__
#endif
#if !defined(__device__)
#define __device__
#endif
#endif
