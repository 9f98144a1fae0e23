// Shared by the translation units behind the extern "C" boundary: capi.hip, samplers.hip, test_ops.hip.
#pragma once
#include "unet_engine.h"

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
// every image of a sampler step shares the step time: the engine computes ONE embedding row (stride-0 broadcast)
inline UnetRun uniform_t_run() { UnetRun r; r.t_uniform = 1; return r; }
